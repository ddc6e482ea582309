# stream_harness.cpp on top of the objects of Makefile (same flags, same fake runtime): make -f stream.mk OUT=... $(OUT)/stream_harness.
# Like wind_harness.cpp it reads the launch arguments (KParams, Arrays: kernels.h), so it is compiled as host-only HIP like the units.
include Makefile

$(OUT)/stream_harness: stream_harness.cpp fake_hip.cpp $(OBJS) $(OUT)/fatbin_stub.c
	$(HIPCC) $(HFLAGS) -x hip -c stream_harness.cpp -o $(OUT)/stream_harness.host.o
	$(CXX_) -std=c++17 $(SAN) -I/opt/rocm/include -rdynamic fake_hip.cpp $(OUT)/fatbin_stub.c -x none $(OBJS) $(OUT)/stream_harness.host.o -o $@ -ldl -lpthread

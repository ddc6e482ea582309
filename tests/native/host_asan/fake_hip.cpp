// fake_hip.cpp — a HOST-ONLY stand-in for the HIP runtime, for ONE purpose: running the host side of libpicles_hip.so
// (the C ABI of include/picles_hip.h: allocation sizes, copies across the ABI, re-packing, rings, stores, event / stream
// lifetimes) under AddressSanitizer on a box without a GPU.  "Device" memory is ordinary heap memory, so every
// hipMemcpy / hipMemset the library issues is checked by ASan against the size of BOTH buffers; kernel launches are
// accepted and do nothing (the numbers that come back are meaningless and nothing here looks at them).  Streams and
// events are small heap objects: a use after destroy or a double destroy is reported.
// Two switches for the harnesses:
//   * PICLES_FAKE_HIP_TRACE=<file>: every runtime entry point appends one line — its name, the streams and events involved as
//     ordinals in order of creation (s0 = the null stream; never pointers), byte counts and copy kinds, kernel name, grid and block
//     of a launch.  Two builds of the library that enqueue, wait, record and synchronise alike give the same lines but for the
//     alloc / free / create / destroy ones.  Ordinals count per thread; a thread other than the main one keeps its lines and
//     appends them as one block ("thread {" ... "}") when it ends, so the blocks of concurrent ranks never interleave (their order
//     among each other is the only thing left to chance).
//   * fake_hip_fail_alloc(k): the k-th next hipMalloc / hipHostMalloc / event or stream creation fails, once (k <= 0: off); returns
//     what was left of the previous count (> 0: that failure never came).  fake_hip_live(): device and pinned blocks plus events
//     alive now — a failed call that gives the same number back as before has left nothing behind.
//   * fake_hip_launch_hook(f): f (nullptr: none) is called at every kernel launch with the kernel's (mangled) name and its argument
//     array, behind the launch's own trace line; fake_hip_trace_line(text) lets it append a line of its own to the trace.
// TEST INFRASTRUCTURE ONLY (tests/test_host_asan.py).  Never linked into, shipped with or loaded by the product.
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>

namespace {
struct FakeStream { unsigned magic; int id; };
struct FakeEvent { unsigned magic; bool recorded; int id; };
constexpr unsigned SM = 0x57AEA11u, EM = 0xE7E47u;
thread_local hipError_t t_last = hipSuccess;
hipError_t fail(hipError_t e) { t_last = e; return e; }
bool ok_stream(hipStream_t s) { return s == nullptr || reinterpret_cast<FakeStream *>(s)->magic == SM; }   /* a freed stream: ASan reports the read */

/* ---- the trace ---- */
const std::thread::id g_main = std::this_thread::get_id();
std::mutex g_trace_mu;
FILE *trace_file()
{
    static FILE *f = [] { const char *p = getenv("PICLES_FAKE_HIP_TRACE"); return (p && *p) ? fopen(p, "a") : (FILE *)nullptr; }();
    return f;
}
struct ThreadLines {
    std::string text;
    ~ThreadLines()
    {
        if (text.empty() || !trace_file()) return;
        std::lock_guard<std::mutex> lk(g_trace_mu);
        fprintf(trace_file(), "thread {\n%s}\n", text.c_str());
        fflush(trace_file());
    }
};
thread_local ThreadLines t_lines;
thread_local int t_streams = 0, t_events = 0;
void trace(const char *fmt, ...)
{
    FILE *f = trace_file();
    if (!f) return;
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (std::this_thread::get_id() == g_main) {
        std::lock_guard<std::mutex> lk(g_trace_mu);
        fprintf(f, "%s\n", buf);
        fflush(f);
    } else {
        t_lines.text += buf;
        t_lines.text += '\n';
    }
}
int sid(hipStream_t s) { return s ? reinterpret_cast<FakeStream *>(s)->id : 0; }
int eid(hipEvent_t e) { return reinterpret_cast<FakeEvent *>(e)->id; }
const char *kind_name(hipMemcpyKind k)
{
    switch (k) {
    case hipMemcpyHostToHost: return "H2H";
    case hipMemcpyHostToDevice: return "H2D";
    case hipMemcpyDeviceToHost: return "D2H";
    case hipMemcpyDeviceToDevice: return "D2D";
    default: return "default";
    }
}
std::map<const void *, std::string> &kernel_names() { static std::map<const void *, std::string> m; return m; }

/* ---- the allocation that fails ---- */
std::atomic<long> g_fail_in{0}, g_live{0};
bool alloc_fails()
{
    if (g_fail_in.load() <= 0) return false;
    return g_fail_in.fetch_sub(1) == 1;
}
void *fake_alloc(size_t n)
{
    void *p = alloc_fails() ? nullptr : malloc(n ? n : 1);
    if (p) g_live++;
    return p;
}
void fake_free(void *p)
{
    if (p) g_live--;
    free(p);
}
}

extern "C" long fake_hip_fail_alloc(long k) { return g_fail_in.exchange(k); }
extern "C" long fake_hip_live(void) { return g_live.load(); }
typedef void (*fake_hip_hook)(const char *kernel, void **args);
static fake_hip_hook g_launch_hook = nullptr;
extern "C" void fake_hip_launch_hook(fake_hip_hook f) { g_launch_hook = f; }
extern "C" void fake_hip_trace_line(const char *text) { trace("%s", text); }

extern "C" {
hipError_t hipGetDeviceCount(int *n) { *n = 1; return hipSuccess; }
hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : fail(hipErrorInvalidDevice); }
hipError_t hipGetDevice(int *d) { *d = 0; return hipSuccess; }
hipError_t hipDeviceSynchronize(void) { trace("hipDeviceSynchronize"); return hipSuccess; }
hipError_t hipGetLastError(void) { hipError_t e = t_last; t_last = hipSuccess; return e; }
const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake HIP error"; }
hipError_t hipDeviceGetAttribute(int *v, hipDeviceAttribute_t a, int)
{
    switch (a) {
    case hipDeviceAttributeWarpSize: *v = 64; break;
    case hipDeviceAttributeMultiprocessorCount: *v = 256; break;
    case hipDeviceAttributeMaxThreadsPerBlock: *v = 1024; break;
    case hipDeviceAttributeMaxSharedMemoryPerBlock: *v = 65536; break;
    default: *v = 1024;
    }
    return hipSuccess;
}
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600 *p, int)
{
    memset(p, 0, sizeof(*p));
    snprintf(p->name, sizeof(p->name), "fake gfx950");
    snprintf(p->gcnArchName, sizeof(p->gcnArchName), "gfx950");
    p->warpSize = 64; p->multiProcessorCount = 256; p->maxThreadsPerBlock = 1024; p->sharedMemPerBlock = 65536;
    p->maxThreadsPerMultiProcessor = 2048; p->regsPerBlock = 65536; p->totalGlobalMem = (size_t)1 << 36;
    p->maxGridSize[0] = p->maxGridSize[1] = p->maxGridSize[2] = 0x7fffffff;
    p->maxThreadsDim[0] = p->maxThreadsDim[1] = p->maxThreadsDim[2] = 1024;
    return hipSuccess;
}
int hipGetStreamDeviceId(hipStream_t s) { (void)ok_stream(s); return 0; }

hipError_t hipMalloc(void **p, size_t n)
{
    trace("hipMalloc %zu", n);
    *p = fake_alloc(n);
    return *p ? hipSuccess : fail(hipErrorOutOfMemory);
}
hipError_t hipFree(void *p) { trace("hipFree"); fake_free(p); return hipSuccess; }
hipError_t hipHostMalloc(void **p, size_t n, unsigned)
{
    trace("hipHostMalloc %zu", n);
    *p = fake_alloc(n);
    return *p ? hipSuccess : fail(hipErrorOutOfMemory);
}
hipError_t hipHostFree(void *p) { trace("hipHostFree"); fake_free(p); return hipSuccess; }
hipError_t hipHostGetDevicePointer(void **d, void *h, unsigned) { *d = h; return hipSuccess; }
hipError_t hipMemcpy(void *d, const void *s, size_t n, hipMemcpyKind k)
{
    trace("hipMemcpy %zu %s", n, kind_name(k));
    memmove(d, s, n);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *d, const void *s, size_t n, hipMemcpyKind k, hipStream_t st)
{
    if (!ok_stream(st)) return fail(hipErrorInvalidHandle);
    trace("hipMemcpyAsync %zu %s s%d", n, kind_name(k), sid(st));
    memmove(d, s, n);
    return hipSuccess;
}
hipError_t hipMemset(void *d, int v, size_t n) { trace("hipMemset %zu", n); memset(d, v, n); return hipSuccess; }
hipError_t hipMemsetAsync(void *d, int v, size_t n, hipStream_t st)
{
    if (!ok_stream(st)) return fail(hipErrorInvalidHandle);
    trace("hipMemsetAsync %zu s%d", n, sid(st));
    memset(d, v, n);
    return hipSuccess;
}

hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned)
{
    if (alloc_fails()) { *s = nullptr; trace("hipStreamCreate failed"); return fail(hipErrorOutOfMemory); }
    FakeStream *f = new FakeStream{SM, ++t_streams};
    trace("hipStreamCreate s%d", f->id);
    *s = reinterpret_cast<hipStream_t>(f);
    return hipSuccess;
}
hipError_t hipStreamDestroy(hipStream_t s)
{
    FakeStream *f = reinterpret_cast<FakeStream *>(s);
    if (!f || f->magic != SM) return fail(hipErrorInvalidHandle);
    trace("hipStreamDestroy s%d", f->id);
    f->magic = 0;
    delete f;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t s)
{
    if (!ok_stream(s)) return fail(hipErrorInvalidHandle);
    trace("hipStreamSynchronize s%d", sid(s));
    return hipSuccess;
}
hipError_t hipStreamQuery(hipStream_t s)
{
    if (!ok_stream(s)) return fail(hipErrorInvalidHandle);
    trace("hipStreamQuery s%d", sid(s));
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned)
{
    if (alloc_fails()) { *e = nullptr; trace("hipEventCreate failed"); return fail(hipErrorOutOfMemory); }
    FakeEvent *f = new FakeEvent{EM, false, ++t_events};
    g_live++;
    trace("hipEventCreate e%d", f->id);
    *e = reinterpret_cast<hipEvent_t>(f);
    return hipSuccess;
}
hipError_t hipEventCreate(hipEvent_t *e) { return hipEventCreateWithFlags(e, 0); }
hipError_t hipEventDestroy(hipEvent_t e)
{
    FakeEvent *f = reinterpret_cast<FakeEvent *>(e);
    if (!f || f->magic != EM) return fail(hipErrorInvalidHandle);
    trace("hipEventDestroy e%d", f->id);
    g_live--;
    f->magic = 0;
    delete f;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t e, hipStream_t s)
{
    FakeEvent *f = reinterpret_cast<FakeEvent *>(e);
    if (!f || f->magic != EM || !ok_stream(s)) return fail(hipErrorInvalidHandle);
    trace("hipEventRecord e%d s%d", f->id, sid(s));
    f->recorded = true;
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t e)
{
    if (reinterpret_cast<FakeEvent *>(e)->magic != EM) return fail(hipErrorInvalidHandle);
    trace("hipEventSynchronize e%d", eid(e));
    return hipSuccess;
}
hipError_t hipEventElapsedTime(float *ms, hipEvent_t a, hipEvent_t b)
{
    if (reinterpret_cast<FakeEvent *>(a)->magic != EM || reinterpret_cast<FakeEvent *>(b)->magic != EM) return fail(hipErrorInvalidHandle);
    trace("hipEventElapsedTime e%d e%d", eid(a), eid(b));
    *ms = 0.125f;
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned)
{
    if (!(ok_stream(s) && reinterpret_cast<FakeEvent *>(e)->magic == EM)) return fail(hipErrorInvalidHandle);
    trace("hipStreamWaitEvent s%d e%d", sid(s), eid(e));
    return hipSuccess;
}

/* kernel launches: accepted, not executed */
hipError_t hipLaunchKernel(const void *fn, dim3 grid, dim3 block, void **args, size_t, hipStream_t s)
{
    if (!ok_stream(s)) return fail(hipErrorInvalidHandle);
    if (trace_file() || g_launch_hook) {
        std::string name = "?";
        {
            std::lock_guard<std::mutex> lk(g_trace_mu);
            auto it = kernel_names().find(fn);
            if (it != kernel_names().end()) name = it->second;
        }
        trace("hipLaunchKernel %s grid %u,%u,%u block %u,%u,%u s%d", name.c_str(), grid.x, grid.y, grid.z, block.x, block.y, block.z, sid(s));
        if (g_launch_hook) g_launch_hook(name.c_str(), args);
    }
    if (grid.x == 0 || grid.y == 0 || grid.z == 0 || block.x == 0 || block.x * block.y * block.z > 1024) return fail(hipErrorInvalidConfiguration);
    return hipSuccess;
}
struct CallCfg { dim3 g, b; size_t shm; hipStream_t s; };
static thread_local CallCfg t_cfg;
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t shm, hipStream_t s) { t_cfg = {g, b, shm, s}; return hipSuccess; }
hipError_t __hipPopCallConfiguration(dim3 *g, dim3 *b, size_t *shm, hipStream_t *s) { *g = t_cfg.g; *b = t_cfg.b; *shm = t_cfg.shm; *s = t_cfg.s; return hipSuccess; }
void **__hipRegisterFatBinary(const void *) { static void *h; return &h; }
void __hipRegisterFunction(void **, const void *host_fn, char *, const char *device_name, unsigned, void *, void *, void *, void *, int *)
{
    std::lock_guard<std::mutex> lk(g_trace_mu);
    kernel_names()[host_fn] = device_name ? device_name : "?";
}
void __hipRegisterVar(void **, void *, char *, const char *, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void **) {}
}

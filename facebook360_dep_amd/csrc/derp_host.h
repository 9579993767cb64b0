// Host plumbing shared by the C-ABI's handles (derp_ctx, derp_isp, derp_sim): the owning device buffer, the two error
// channels, the HIP / allocation / launch checks, block counts, the create functions' device check and the synchronous
// copies. A handle `h` serves them through h->stream and h->errSink(). Included by derp_capi.hip before its users.
#pragma once

namespace {

// A device allocation and its owner: move-only, freed when the owner dies
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) {
    o.p = nullptr;
    o.bytes = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      bytes = o.bytes;
      o.p = nullptr;
      o.bytes = 0;
    }
    return *this;
  }
  ~DevBuf() {
    release();
  }
  // grow-only; the contents are lost on growth; non-zero (and an empty buffer) when the allocation fails
  int ensure(size_t n) {
    if (n <= bytes) {
      return 0;
    }
    release();
    if (hipMalloc(&p, n) != hipSuccess) {
      p = nullptr;
      return 1;
    }
    bytes = n;
    return 0;
  }
  void release() {
    if (p) {
      (void)hipFree(p);
    }
    p = nullptr;
    bytes = 0;
  }
  template <typename T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

// ---- errors: a handle's own text (derp_last_error(handle)) or the calling thread's (derp_last_error(nullptr)), where
// the create functions and every derp_isp_* / derp_sim_* call report ----
thread_local std::string g_create_error;

int vfail(std::string* sink, const char* fmt, va_list ap) {
  char buf[512];
  vsnprintf(buf, sizeof buf, fmt, ap);
  if (sink) {
    *sink = buf;
  }
  return 1;
}
int fail(std::string* sink, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vfail(sink, fmt, ap);
  va_end(ap);
  return 1;
}
int create_fail(const std::string& m) {
  g_create_error = m;
  return 1;
}

#define HIPCHK(h, expr)                                                                                            \
  do {                                                                                                             \
    hipError_t e_ = (expr);                                                                                        \
    if (e_ != hipSuccess) {                                                                                        \
      return fail((h)->errSink(), "HIP error %s at %s:%d (%s)", hipGetErrorString(e_), __FILE__, __LINE__, #expr); \
    }                                                                                                              \
  } while (0)
#define ALLOC(h, buf, n)                                                                                    \
  do {                                                                                                      \
    if ((buf).ensure(n)) {                                                                                  \
      return fail((h)->errSink(), "out of device memory allocating %zu bytes (%s)", (size_t)(n), #buf);      \
    }                                                                                                       \
  } while (0)
#define KCHECK(h) HIPCHK(h, hipGetLastError())  // after a launch (or several): did the runtime accept them
#define TRY(expr)       \
  do {                  \
    int r_ = (expr);    \
    if (r_) {           \
      return r_;        \
    }                   \
  } while (0)

// ---- launch geometry ----
dim3 grid2d(int w, int h, int z, dim3 b) {
  return dim3((w + b.x - 1) / b.x, (h + b.y - 1) / b.y, z);
}
const dim3 kBlk2d(32, 8, 1);

unsigned blocks_of(size_t n, size_t block) {
  return (unsigned)((n + block - 1) / block);
}
// blocks of 256 for a grid-stride kernel: capped
int flat_grid(size_t n) {
  return (int)std::min<size_t>((n + 255) / 256, 2048 * 4);
}

// ---- what every *_create checks before it touches the device: a HIP device, the index, gfx950 (or
// DERP_ALLOW_ANY_ARCH). `path` names what has no CPU fallback. ----
int open_device(int device, const char* path, hipDeviceProp_t* prop) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    return create_fail(std::string("no HIP device present: ") + path + " has no CPU fallback");
  }
  if (device < 0 || device >= count) {
    return create_fail("HIP device index out of range");
  }
  if (hipGetDeviceProperties(prop, device) != hipSuccess) {
    return create_fail("hipGetDeviceProperties failed");
  }
  if (strncmp(prop->gcnArchName, "gfx950", 6) != 0 && !getenv("DERP_ALLOW_ANY_ARCH")) {
    return create_fail(std::string("device is ") + prop->gcnArchName + ", this library is built for gfx950 only");
  }
  if (hipSetDevice(device) != hipSuccess) {
    return create_fail("hipSetDevice failed");
  }
  return 0;
}

// The host-pointer entry points copy with plain hipMemcpy: a handle's stream is non-blocking, so these null-stream
// copies do not order against it — a kernel's input is complete when the call returns, its output is read after a
// synchronise (and after asking whether the launches before it were accepted: the launch check of those entry points).
template <typename Handle>
int upload_sync(Handle* h, DevBuf& buf, const void* host, size_t bytes) {
  ALLOC(h, buf, bytes);
  HIPCHK(h, hipMemcpy(buf.p, host, bytes, hipMemcpyHostToDevice));
  return 0;
}
template <typename Handle>
int download_sync(Handle* h, void* host, const void* dev, size_t bytes) {
  KCHECK(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost));
  return 0;
}

}  // namespace

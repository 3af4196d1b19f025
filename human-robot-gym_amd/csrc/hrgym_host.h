// hrgym_host.h -- what the host files of the library share.  The first part is for every translation unit (the two hull units' test taps use it): the hull
// centroids and the host side of a test tap.  The rest belongs to the base unit, which holds the C ABI (include/hrgym.h) in the three files it includes behind this
// one: hrgym_host_batch.h (hrg_batch_*, hrg_debug_*), hrgym_host_buffers.h (hrg_her_*, hrg_rollout_*, hrg_replay_*) and hrgym_host_learners.h (hrg_sac_*, hrg_ppo_*,
// hrg_eval_*).  Here: the error string, a handle's device memory (DeviceMem) and how a handle is destroyed, and what the entries share of launching and exporting.
#pragma once
#include <type_traits>

// vertex centroid of each hull (body frame): the interior point MPR starts from (hrg_batch_create, hrg_test_hull_box_queries)
static inline void hull_centroids(const double* verts, const int32_t* off, double cen[HRG_NHULL][3]) {
  for (int h = 0; h < HRG_NHULL; h++) {
    double s[3] = {0, 0, 0};
    for (int i = off[h]; i < off[h + 1]; i++) for (int a = 0; a < 3; a++) s[a] += verts[3 * i + a];
    for (int a = 0; a < 3; a++) cen[h][a] = s[a] / (double)(off[h + 1] - off[h]);
  }
}

// host side of a test tap (hrg_test_hull_queries, hrg_test_hull_box_queries, hrg_debug_pose_compare): the n_in host buffers copied to the device, one launch, the
// output copied back.  launch(d) gets the device buffers, d[0 .. n_in - 1] the inputs in order and d[n_in] the output; all of them are freed on every path.
struct TapBuf { const void* host; size_t bytes; };
template <class Launch>
static bool hrg_run_tap(const TapBuf* in, int n_in, void* out_host, size_t out_bytes, Launch launch) {
  void* d[8] = {nullptr};
  bool ok = n_in < 8;
  for (int i = 0; ok && i < n_in; i++) ok = hipMalloc(&d[i], in[i].bytes) == hipSuccess && hipMemcpy(d[i], in[i].host, in[i].bytes, hipMemcpyHostToDevice) == hipSuccess;
  if (ok && hipMalloc(&d[n_in], out_bytes) == hipSuccess) {
    launch(d);
    ok = hipDeviceSynchronize() == hipSuccess && hipMemcpy(out_host, d[n_in], out_bytes, hipMemcpyDeviceToHost) == hipSuccess;
  } else ok = false;
  for (int i = 0; i < 8; i++) hipFree(d[i]);
  return ok;
}

#if HRG_BASE_TU
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x)                                                                                         \
  do {                                                                                                    \
    hipError_t _e = (x);                                                                                  \
    if (_e != hipSuccess) return fail(HRG_ERR_HIP, std::string(#x) + ": " + hipGetErrorString(_e));        \
  } while (0)

extern "C" const char* hrg_last_error(void) { return g_err.c_str(); }

// what a test tap of the base unit returns: `ok` of hrg_run_tap, `name` the entry's
static int tap_result(bool ok, const char* name) { return ok ? HRG_OK : fail(HRG_ERR_HIP, std::string(name) + ": device allocation / copy / launch failed"); }

// every device allocation of one handle: zeroed or uploaded, counted, freed together
struct DeviceMem {
  std::vector<void*> ptrs;
  size_t bytes = 0;    // device memory held
  size_t failed = 0;   // the request the device refused
  DeviceMem() = default;
  DeviceMem(const DeviceMem&) = delete;
  DeviceMem& operator=(const DeviceMem&) = delete;
  ~DeviceMem() {
    for (void* p : ptrs) hipFree(p);
  }
  // `count` values behind `out`, zeroed or (upload) copied from `host`; false where the device refuses (HIP's sticky error is cleared, `failed` is the request)
  template <class T> bool zeros(T*& out, size_t count) { return filled(out, nullptr, count); }
  template <class T> bool upload(T*& out, const typename std::remove_const<T>::type* host, size_t count) { return filled(out, host, count); }
  template <class T> bool filled(T*& out, const void* host, size_t count) {
    const size_t b = count * sizeof(T);
    void* p = nullptr;
    if (hipMalloc(&p, b) != hipSuccess) p = nullptr;
    if (p) ptrs.push_back(p);
    if (!p || (host ? hipMemcpy(p, host, b, hipMemcpyHostToDevice) : hipMemset(p, 0, b)) != hipSuccess) {
      (void)hipGetLastError();
      failed = b;
      return false;
    }
    bytes += b;
    out = (T*)p;
    return true;
  }
};

static int nomem(const char* name, const DeviceMem& mem) {
  return fail(HRG_ERR_NOMEM, std::string(name) + ": device allocation of " + std::to_string(mem.failed) + " bytes failed");
}

// hrg_*_destroy of a handle with `device` (its DeviceMem member frees what it holds)
template <class H> static void destroy_handle(H* h) {
  if (!h) return;
  hipSetDevice(h->device);
  hipDeviceSynchronize();
  delete h;
}

// Pieces of one zeroed allocation of T, handed out in order: take(p, n) asks for n values behind p, alloc() makes the allocation and sets every pointer asked for
template <class T> struct Carver {
  std::vector<std::pair<T**, size_t>> pieces;   // where the pointer goes, the piece's first value
  size_t count = 0;
  void take(T*& out, size_t n) {
    pieces.push_back({&out, count});
    count += n;
  }
  bool alloc(DeviceMem& mem) {
    T* base = nullptr;
    if (!mem.zeros(base, count)) return false;
    for (const auto& p : pieces) *p.first = base + p.second;
    return true;
  }
};

// hrg_*_export of a learner: once the device is idle, every array the caller asked for (a non-null `host`) to the host
struct ExportFloats {
  float* host;
  const float* dev;
  size_t count;
};
static int export_floats(int device, std::initializer_list<ExportFloats> arrays) {
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipDeviceSynchronize());
  for (const ExportFloats& a : arrays)
    if (a.host) HIPCHK(hipMemcpy(a.host, a.dev, a.count * sizeof(float), hipMemcpyDeviceToHost));
  return HRG_OK;
}

// hrg_*_stats: the tracker's sums [n_envs][cols] to the host, cleared on the device on request
static int buffer_stats(int device, double* acc_dev, int32_t n_envs, int cols, double* per_env_host, int32_t clear) {
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipDeviceSynchronize());
  const size_t bytes = sizeof(double) * (size_t)cols * (size_t)n_envs;
  HIPCHK(hipMemcpy(per_env_host, acc_dev, bytes, hipMemcpyDeviceToHost));
  if (clear) {
    HIPCHK(hipMemset(acc_dev, 0, bytes));
    HIPCHK(hipDeviceSynchronize());
  }
  return HRG_OK;
}

// the two grids of the buffer kernels: a wavefront per env, and blocks of four wavefronts with one of `n` rows, samples or indices each
template <class K, class... A> static int launch_per_env(K kernel, int32_t n_envs, void* stream, A... args) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_envs), dim3(64), 0, (hipStream_t)stream, args...);
  HIPCHK(hipGetLastError());
  return HRG_OK;
}
template <class K, class... A> static int launch_per_wave(K kernel, int32_t n, void* stream, A... args) {
  const unsigned per = HRG_BUFFER_BLOCK / 64;
  hipLaunchKernelGGL(kernel, dim3(((unsigned)n + per - 1) / per), dim3(HRG_BUFFER_BLOCK), 0, (hipStream_t)stream, args...);
  HIPCHK(hipGetLastError());
  return HRG_OK;
}
#endif // HRG_BASE_TU

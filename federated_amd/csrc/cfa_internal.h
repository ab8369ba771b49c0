// cfa_internal.h — shared internals of libcfa's translation units (not installed, not an ABI).
//
// Device helpers for gfx950 (MI355X / CDNA4): the float4 streaming loads and stores, ONE
// definition of each mixing rule's step (seq_step, div_step, lin_step, tf1_first / tf1_step,
// div_step_f64, mewma_step, mewma_step_f64, split_sum) that every kernel of the library calls,
// the fold of the sequential / linear / FedAvg rules, the tile walk (TileWalk) and the fan-in
// dispatch (dispatch_fanin) of the streaming kernels, the compression epilogue, what the rounds
// of cfa_population.hip and cfa_fedavg.hip share (SchedArgs, sched_slot, first_flagged), and the
// thread-local error reporting behind cfa_last_error(). The host-only launch rules (shape bands,
// bucket split, passes) are in cfa_mix_shape.h. Every .hip file of the library
// is compiled with -ffp-contract=off: CFA_RULE_SEQUENTIAL evaluates t = x - w; t = a * t;
// w = w + t exactly as fp32 numpy does (three roundings), which makes the TF2 path
// bit-identical to the reference; CFA_RULE_LINEAR uses explicit fmaf.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>

#include "cfa_engine.h"
#include "cfa_mix_shape.h"

typedef float f4 __attribute__((ext_vector_type(4)));
typedef unsigned u4v __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------
// Error reporting: one thread-local message per thread, shared by the library's translation
// units (C++17 inline variable); no global mutable state is shared between threads.
// ------------------------------------------------------------------------------------------
inline thread_local std::string g_last_error;

__attribute__((format(printf, 2, 3))) inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

#define CFA_HIP_CHECK(expr)                                                              \
  do {                                                                                   \
    hipError_t e_ = (expr);                                                              \
    if (e_ != hipSuccess)                                                                \
      return fail(CFA_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),      \
                  __FILE__, __LINE__);                                                   \
  } while (0)

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(CFA_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
  return CFA_OK;
}

namespace {

constexpr int kBlock = 256;  // 4 waves of 64 lanes

// Default launch configuration (cfa_launch_t), optionally overridden once from the
// environment (CFA_BLOCKS_PER_CU, CFA_VEC_PER_LANE, CFA_NONTEMPORAL); immutable after first use.
// Explicit per-call configurations go through cfa_mix_seq_ex_f32.
// Defaults from the in-process sweep on MI355X (tools/tune_mix.py, profiles/r01_tune.jsonl):
// 2 resident workgroups per CU with a grid-stride loop, nontemporal loads and stores, and
// vec_per_lane = 0 (auto: the widest tile that keeps (n+1)*vec <= 40 float4 in registers); the
// streaming mix kernel has its own default below.
// blocks_per_cu = kAutoBlocks in the library default means "per kernel": the streaming mix
// kernel takes its own shape (mix_auto_shape), every other kernel kDefaultBlocks.
constexpr int kDefaultBlocks = 2;
constexpr int kAutoBlocks = -1;
static cfa_launch_t read_tune() {
  cfa_launch_t t{kAutoBlocks, 0, 1};
  if (const char* s = getenv("CFA_BLOCKS_PER_CU")) {
    const int v = atoi(s);  // 0 = one workgroup per tile, > 0 = cap per CU; negative = the default
    t.blocks_per_cu = v >= 0 ? v : kAutoBlocks;
  }
  if (const char* s = getenv("CFA_VEC_PER_LANE")) t.vec_per_lane = norm_vec(atoi(s));
  if (const char* s = getenv("CFA_NONTEMPORAL")) t.nontemporal = atoi(s) ? 1 : 0;
  return t;
}
static const cfa_launch_t& tune() {
  static const cfa_launch_t t = read_tune();  // C++11 magic static: thread-safe init
  // CFA_TUNE_DYNAMIC=1 (measurement tools only): re-read the environment at every launch, so one
  // process can compare launch shapes on the same buffers (tools/probe/tune_entries.py)
  static const bool dynamic = getenv("CFA_TUNE_DYNAMIC") != nullptr;
  if (dynamic) {
    thread_local cfa_launch_t d;
    d = read_tune();
    return d;
  }
  return t;
}

}  // namespace

// Per-device attributes, cached after the first query: the CU count and the LDS a workgroup may
// take. Inline functions with external linkage, so every translation unit shares one cache;
// cfa_device_prepare() fills it before any launch (the launch path then only reads it, which keeps
// hipGraph capture free of device queries). A failed query gives `fallback`, and caches it when
// `keep_fallback` (the LDS size; a failed CU-count query is asked again).
inline int device_attr(int slot, hipDeviceAttribute_t attr, int fallback, bool keep_fallback) {
  static int cache[2][64] = {{0}};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return fallback;
  if (dev >= 0 && dev < 64) {
    const int c = __atomic_load_n(&cache[slot][dev], __ATOMIC_RELAXED);
    if (c > 0) return c;
  }
  int v = 0;
  if (hipDeviceGetAttribute(&v, attr, dev) != hipSuccess || v <= 0) {
    if (!keep_fallback) return fallback;
    v = fallback;
  }
  if (dev >= 0 && dev < 64) __atomic_store_n(&cache[slot][dev], v, __ATOMIC_RELAXED);
  return v;
}
inline int device_cus() { return device_attr(0, hipDeviceAttributeMultiprocessorCount, 256, false); }
// Dynamic LDS for one workgroup: up to 64 KiB by default; above that a kernel's limit is raised
// to the device's (160 KiB on gfx950) when the runtime allows it (cfa_grad.hip).
inline int device_lds_max() { return device_attr(1, hipDeviceAttributeMaxSharedMemoryPerBlock, 65536, true); }

// cfa_grad.hip: per-device LDS query and kernel LDS limits, done ahead of any capture.
int grad_prepare_device();
// cfa_local_sgd.hip: the same for the local-SGD kernels.
int local_sgd_prepare_device();
// cfa_lenet.hip: the same for the LeNet-family evaluation kernels.
int lenet_prepare_device();
// cfa_lenet_grad.hip: the LeNet-family gradient kernels (called by lenet_prepare_device).
int lenet_grad_prepare_device();
// cfa_lenet_max.hip: the max-pool kernels of the same family (called by lenet_prepare_device).
int lenet_max_prepare_device();
// cfa_lenet_hidden.hip: the hidden-layer kernels of the same family (called by lenet_prepare_device).
int lenet_hidden_prepare_device();
// cfa_ring.hip: the sliding ring round's seam kernels (those that keep more than 64 KiB of rows).
int ring_prepare_device();
// cfa_population.hip: one-thread launch that leaves a device counter (a schedule's round, a cost
// log's epoch) one higher, in stream order.
int advance_counter(unsigned long long* counter, hipStream_t st);

namespace {

static unsigned grid_for(long long tiles, const cfa_launch_t& t = tune()) {
  if (tiles <= 0) return 1;
  long long g = tiles;
  const int bpc = t.blocks_per_cu == kAutoBlocks ? kDefaultBlocks : t.blocks_per_cu;
  if (bpc > 0) {
    long long cap = (long long)device_cus() * bpc;
    if (g > cap) g = cap;
  }
  if (g > 0x7fffffffLL) g = 0x7fffffffLL;
  return (unsigned)g;
}

// grid_for with a kernel's own default workgroups per CU, used while the launch configuration is
// the library default (an explicit CFA_BLOCKS_PER_CU applies to every kernel alike).
static unsigned grid_for_own(long long tiles, int own_blocks_per_cu) {
  cfa_launch_t t = tune();
  if (t.blocks_per_cu == kAutoBlocks) t.blocks_per_cu = own_blocks_per_cu;
  return grid_for(tiles, t);
}

// grid.x of a launch whose gy rows of workgroups (grid.y) share the device: about wg_per_cu
// workgroups per CU over all rows, at most one per tile, at least one.
static unsigned shared_grid_x(long long tiles, int wg_per_cu, long long gy) {
  long long gx = ((long long)device_cus() * wg_per_cu + gy - 1) / gy;
  if (gx > tiles) gx = tiles;
  if (gx < 1) gx = 1;
  return (unsigned)gx;
}

// An environment override as atoi reads it (0 for text that is no number); `unset` without one.
static int env_int(const char* name, int unset) {
  const char* s = getenv(name);
  return s ? atoi(s) : unset;
}

// Kernel-argument pack: pointers + coefficients land in SGPRs.
struct Fanin {
  const float* src[CFA_MAX_FANIN + 1];  // [0] = local (w0), [1..N] = neighbours
  float c[CFA_MAX_FANIN + 1];           // SEQ: c[j] = alpha of src[j] (c[0] unused); LIN: coeff
  float d[CFA_MAX_FANIN + 1];           // SEQ_DIV: d[j] = divisor of step j (d[0] unused)
  double rd[CFA_MAX_FANIN + 1];         // SEQ_DIV: rd[j] = RN_64(1 / d[j]) (div4_rn)
};

// Correctly rounded fp32 a / b as one fp64 multiply: q = (float)((double)a * RN_64(1/b)) is IEEE
// a / b whenever the exact quotient is not an exact SUBNORMAL rounding midpoint. Away from a
// midpoint the exact quotient of two 24-bit significands lies at least 2^-48 (relative) from it,
// while the two fp64 roundings (of 1/b and of the product) stay within 2^-52: the conversion
// rounds the right way, normal or subnormal, and fp64's exponent range holds every fp32 quotient
// (overflow happens in the conversion as in the IEEE division; zeros, infinities and NaN
// propagate as there). A subnormal quotient has fewer significand bits and CAN sit exactly on a
// midpoint (a = odd k * o * 2^-149, b = 2o): there the fp64 error of RN(1/b) decides the rounding
// instead of ties-to-even (round-4 advisor finding). Such a quotient converts to a subnormal fp32
// (or to 0 only when it is below the 2^-150 tie, which rounds to 0 anyway; the tie below 2^-126
// rounds up to the normal 2^-126, which ties-to-even also gives), so each step records whether
// any of its results is subnormal (one v_cmp_class per element, OR-ed on the scalar unit), and a
// fold that saw one redoes its tile with the IEEE division (fold below: one exec-masked branch per
// tile, never taken on the bench's buckets). Round 4 replaced Markstein's three fp32 operations
// plus a range test per float4 with the one-multiply form (profiles/r04_div64_sweep.jsonl: 0.733
// -> 0.776 of peak at 25M, n = 8). Tested bit for bit against numpy over every binade and on exact
// subnormal ties (tests/test_gpu_kernels.py test_mix_seq_div_*; the rule itself on the CPU,
// tests/test_div64_rule.py).
constexpr int kFcSubnormal = 0x0090;  // __builtin_isfpclass: negative | positive subnormal
__device__ __forceinline__ f4 div4_rn(f4 a, double rb, bool& subnormal) {
  f4 q;
  q.x = (float)((double)a.x * rb);
  q.y = (float)((double)a.y * rb);
  q.z = (float)((double)a.z * rb);
  q.w = (float)((double)a.w * rb);
  subnormal = subnormal | __builtin_isfpclass(q.x, kFcSubnormal) | __builtin_isfpclass(q.y, kFcSubnormal) |
              __builtin_isfpclass(q.z, kFcSubnormal) | __builtin_isfpclass(q.w, kFcSubnormal);
  return q;
}
__device__ __forceinline__ f4 div4_ieee(f4 a, float b) {
  f4 q;
  q.x = a.x / b;
  q.y = a.y / b;
  q.z = a.z / b;
  q.w = a.w / b;
  return q;
}

// Host side: fills f.rd from f.d[0..n].
inline void set_reciprocals(Fanin& f, int n) {
  for (int k = 0; k <= n; ++k) f.rd[k] = 1.0 / (double)f.d[k];
}

template <bool NT>
__device__ __forceinline__ f4 ld4(const float* p, long long i) {
  const f4* q = reinterpret_cast<const f4*>(p) + i;
  if constexpr (NT) return __builtin_nontemporal_load(q);
  else return *q;
}
template <bool NT>
__device__ __forceinline__ void st4(float* p, long long i, f4 v) {
  f4* q = reinterpret_cast<f4*>(p) + i;
  if constexpr (NT) __builtin_nontemporal_store(v, q);
  else *q = v;
}

// One step of the sequential rule on a float4 or a float: three separately rounded fp32
// operations (-ffp-contract=off), as fp32 numpy evaluates w + eps * (x - w). Every sequential
// fold of the library steps through here; every bit-for-bit claim rests on it.
template <typename T>
__device__ __forceinline__ T seq_step(T acc, T x, float a) {
  T t = x - acc;   // numpy: (x - w)
  t = a * t;       //        eps * (...)
  return acc + t;  //        w + (...)
}

// One step of the FedAvg divisor rule: t = x - w; t = c * t; t = t / d; w = w + t, the division
// between the multiply and the add (not seq_step). IEEE = false divides a float4 by the fp64
// reciprocal rd (div4_rn, which records a subnormal quotient); IEEE = true is the IEEE division,
// which the redo of such a tile and every scalar kernel take.
template <bool IEEE, typename T>
__device__ __forceinline__ T div_step(T w, T x, float c, float d, double rd, bool& subnormal) {
  T t = x - w;  // numpy: (x - w)
  t = c * t;    //        u * (...)
  if constexpr (!IEEE) t = div4_rn(t, rd, subnormal);  // (...) / C, one fp64 multiply
  else if constexpr (std::is_same_v<T, f4>) t = div4_ieee(t, d);
  else t = t / d;
  return w + t;
}

// One step of the linear closed form: w = fma(c, x, w) per element.
template <typename T>
__device__ __forceinline__ T lin_step(T w, T x, float c) {
  if constexpr (std::is_same_v<T, float>) {
    return fmaf(c, x, w);
  } else {
    w.x = fmaf(c, x.x, w.x);
    w.y = fmaf(c, x.y, w.y);
    w.z = fmaf(c, x.z, w.z);
    w.w = fmaf(c, x.w, w.w);
    return w;
  }
}

// The TF1 chain under numpy 2 (cfa.py:66-76): the first subtraction x_1 - l of two fp32 arrays is
// fp32 (tf1_first; l is the fp32 local, or an fp64 bucket that holds one), every later operation
// fp64 with the fp64 coefficient a = eps * wf_j (tf1_step, which is also the fp64 folds'
// sequential step on an fp64 x).
template <typename L>
__device__ __forceinline__ double tf1_first(L l, float x, double a) {
  const float d = x - (float)l;       // fp32 - fp32 (both operands fp32)
  return (double)l + a * (double)d;  // np.float64 * fp32 -> fp64; fp32 + fp64 -> fp64
}
template <typename X>
__device__ __forceinline__ double tf1_step(double w, X x, double a) {
  return w + a * ((double)x - w);
}

// Correctly rounded fp64 a / b (Markstein): q = RN(a * rb) with rb = RN(1/b) is within 1 ulp,
// the remainder a - b q is exact (one fma), and RN(q + r * rb) is the correctly rounded quotient
// when nothing under- or overflows; |a| in [2^-900, 2^900] and b in [2^-20, 2^20] guarantee
// that, everything else takes the IEEE division. (The fp32 fold's one-multiply form, div4_rn
// above, needs a format twice as wide; fp64 has none on the GPU.)
__device__ __forceinline__ double ddiv_rn(double a, double b, double rb, bool fast) {
  const double aa = __builtin_fabs(a);
  if (fast && aa >= 0x1p-900 && aa <= 0x1p900) {
    const double q = a * rb;
    const double r = __builtin_fma(-q, b, a);
    return __builtin_fma(r, rb, q);
  }
  return a / b;
}
// One fp64 step of the divisor rule, w + (a * (x - w)) / d: through ddiv_rn (r = RN(1 / d), `fast`
// as there), or IEEE = true with the plain division.
template <bool IEEE>
__device__ __forceinline__ double div_step_f64(double w, double x, double a, double d, double r, bool fast) {
  if constexpr (IEEE) return w + (a * (x - w)) / d;
  else return w + ddiv_rn(a * (x - w), d, r, fast);
}

// One neighbour of the CFA-GE gradient step on a float4 or a float (cfa_ge_2stage.py:331-371,
// :593-621): the MEWMA filter s = rho * g + (1 - rho) * s_old (g itself at init, s_old is then not
// read), then W = W - lr * (filtered ? s : g); five separately rounded fp32 operations. Returns
// the new state.
template <typename T>
__device__ __forceinline__ T mewma_step(T& W, T g, const T& s_old, float rho, float one_minus_rho, T lr, bool init,
                                        bool filtered) {
  T s;
  if (init) {
    s = g;
  } else {
    const T t1 = rho * g;  // numpy: rho*g + (1-rho)*s
    const T t2 = one_minus_rho * s_old;
    s = t1 + t2;
  }
  const T u = lr * (filtered ? s : g);
  W = W - u;
  return s;
}

// Python-float scalar times an array, in the array's dtype (numpy 2: the scalar is weak).
__device__ __forceinline__ double scale(double c, double x, bool f32) {
  return f32 ? (double)((float)c * (float)x) : c * x;
}
// The same step on the reference's TF1 arrays with numpy 2 promotion per operation:
//   s_j = rho*g_j + (1-rho)*s_j (or g_j at init), stored in the state array's dtype;
//   W   = W - lr*(filtered ? s_j : g_j).
// Each product is computed in its array's dtype (s32 / g32: the state / gradient arrays are
// fp32); a sum or difference is fp32 only when both operands are fp32, and W stays fp32 (w32) only
// while every update it receives is fp32. Returns the new state.
__device__ __forceinline__ double mewma_step_f64(double& W, bool& w32, double g, const double& s_old, double rho,
                                                 double one_minus_rho, double lr, bool init, bool filtered,
                                                 bool s32, bool g32) {
  double s;
  if (init) {
    s = g;
  } else {
    const double t1 = scale(rho, g, g32);
    const double t2 = scale(one_minus_rho, s_old, s32);
    s = (g32 && s32) ? (double)((float)t1 + (float)t2) : t1 + t2;
  }
  if (s32) s = (double)(float)s;
  const bool u32 = filtered ? s32 : g32;
  const double t = scale(lr, filtered ? s : g, u32);
  if (w32 && u32) {
    W = (double)((float)W - (float)t);
  } else {
    W = W - t;
    w32 = false;
  }
  return s;
}

// Sum of n partial values p[0], p[stride], ... in that order (deterministic): the batch splits of
// a gradient evaluation.
__device__ __forceinline__ float split_sum(const float* p, int n, long long stride) {
  float s = p[0];
  for (int sp = 1; sp < n; ++sp) s += p[(long long)sp * stride];
  return s;
}

// The divisor fold of one float4 with either division: one loop body, instantiated twice by fold.
template <int N, bool IEEE>
__device__ __forceinline__ f4 fold_div(const f4 (&v)[N + 1], const Fanin& f, bool& subnormal) {
  f4 w = v[0];
#pragma unroll
  for (int j = 1; j <= N; ++j) w = div_step<IEEE>(w, v[j], f.c[j], f.d[j], f.rd[j], subnormal);
  return w;
}

template <int N, int RULE>
__device__ __forceinline__ f4 fold(const f4 (&v)[N + 1], const Fanin& f) {
  if constexpr (RULE == CFA_RULE_SEQUENTIAL) {
    f4 w = v[0];
#pragma unroll
    for (int j = 1; j <= N; ++j) w = seq_step(w, v[j], f.c[j]);
    return w;
  } else if constexpr (RULE == CFA_RULE_SEQUENTIAL_DIV) {
    bool subnormal = false;
    f4 w = fold_div<N, false>(v, f, subnormal);
    // a subnormal quotient may be an exact tie: IEEE division
    if (__builtin_expect(subnormal, 0)) w = fold_div<N, true>(v, f, subnormal);
    return w;
  } else {
    f4 w = f.c[0] * v[0];
#pragma unroll
    for (int j = 1; j <= N; ++j) w = lin_step(w, v[j], f.c[j]);
    return w;
  }
}

// The walk of nvec vectors in tiles of kBlock * U by the workgroups of a launch:
//   for (const long long base : tw.full_tiles())  every full tile this workgroup takes, grid-stride;
//       base = the lane's first vector of the tile, its others follow at base + u * kBlock, no guards
//   if (tw.owns_partial()) for (const long long i : tw.partial_tile())  the lane's vectors of the
//       partial last tile, for the one workgroup that owns that tile (full % gridDim.x)
// Each range is its own iterator (the end is a bound), so the loops compile to the plain ones.
template <int U>
struct TileWalk {
  static constexpr long long kTile = (long long)kBlock * U;
  long long nvec, full;  // full: the number of full tiles
  __device__ explicit TileWalk(long long n) : nvec(n), full(n / kTile) {}
  struct Tiles {
    long long t, full;
    __device__ Tiles begin() const { return *this; }
    __device__ long long end() const { return full; }
    __device__ bool operator!=(long long e) const { return t < e; }
    __device__ void operator++() { t += gridDim.x; }
    __device__ long long operator*() const { return t * kTile + threadIdx.x; }
  };
  struct Vectors {
    long long i, nvec;
    __device__ Vectors begin() const { return *this; }
    __device__ long long end() const { return nvec; }
    __device__ bool operator!=(long long e) const { return i < e; }
    __device__ void operator++() { i += kBlock; }
    __device__ long long operator*() const { return i; }
  };
  __device__ Tiles full_tiles() const { return {(long long)blockIdx.x, full}; }
  __device__ bool owns_partial() const { return blockIdx.x == (unsigned)(full % gridDim.x); }
  __device__ Vectors partial_tile() const { return {full * kTile + threadIdx.x, nvec}; }
};

// Run-time fan-in n to compile-time N: fn(std::integral_constant<int, N>{}) for the N in
// LO..CFA_MAX_FANIN equal to n (nothing for an n outside).
template <int LO, typename F, int... Is>
inline void dispatch_fanin_seq(int n, F&& fn, std::integer_sequence<int, Is...>) {
  ((n == LO + Is ? (void)fn(std::integral_constant<int, LO + Is>{}) : (void)0), ...);
}
template <int LO, typename F>
inline void dispatch_fanin(int n, F&& fn) {
  dispatch_fanin_seq<LO>(n, fn, std::make_integer_sequence<int, CFA_MAX_FANIN - LO + 1>{});
}

// Compression epilogue on one element (TF1/consensus/cfa_ongraphs.py:225-273), fp32 arrays.
// numpy 2 (NEP 50) casts the Python-float threshold and replacement to fp32, so the test, the
// product sign(.)*rep and the DPCM sum ref + sign(.)*rep are all fp32 operations (the reference
// reaches this with fp32 arrays when a call has no neighbour, :218-223). sign(0) = 0 and
// sign(NaN) = NaN as numpy. The fp64 variant (compress_one_d) serves the fp64 chains.
__device__ __forceinline__ double np_sign(double x) {
  return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : x);
}
__device__ __forceinline__ float np_signf(float x) {
  return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : x);
}
__device__ __forceinline__ float compress_one(float y, float ref, const CompressParams& cp,
                                              unsigned& kept) {
  const float thr = (float)cp.thr, rep = (float)cp.rep;
  if (cp.mode == CFA_COMPRESS_SPARSE || cp.mode == CFA_COMPRESS_SPARSE_HI) {
    if (fabsf(y) < thr) return np_signf(y) * rep;
  } else if (cp.mode == CFA_COMPRESS_SPARSE_DPCM || cp.mode == CFA_COMPRESS_SPARSE_DPCM_HI) {
    const float d = y - ref;
    if (fabsf(d) < thr) return ref + np_signf(d) * rep;
  }
  ++kept;
  return y;
}

// The same epilogue with the mode's form fixed at compile time (KIND: 0 none, 1 sparse, 2 DPCM;
// compress_kind maps a mode to it) and the thresholds passed in as fp32: straight-line selects
// instead of a per-element branch tree on the runtime mode, which kept the standalone epilogue's
// waves off the memory pipe between tiles (round 4, tools/probe/lowrow_sweep.py). The same fp32
// operations as compress_one, so the same values and count.
__device__ __host__ constexpr int compress_kind(int mode) {
  return (mode == CFA_COMPRESS_SPARSE || mode == CFA_COMPRESS_SPARSE_HI) ? 1
         : (mode == CFA_COMPRESS_SPARSE_DPCM || mode == CFA_COMPRESS_SPARSE_DPCM_HI) ? 2 : 0;
}
template <int KIND>
__device__ __forceinline__ float compress_sel(float y, float ref, float thr, float rep, unsigned& kept) {
  if constexpr (KIND == 0) {
    ++kept;
    return y;
  } else {
    const float d = KIND == 2 ? y - ref : y;
    const bool hit = fabsf(d) < thr;
    const float r = KIND == 2 ? ref + np_signf(d) * rep : np_signf(y) * rep;
    kept += hit ? 0u : 1u;
    return hit ? r : y;
  }
}

// Block-wide sum of one counter per lane, then a single 64-bit atomic per block.
__device__ __forceinline__ void block_add_count(unsigned kept, unsigned long long* dst) {
  __shared__ unsigned red[kBlock / 64];
  unsigned v = kept;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long s = 0;
#pragma unroll
    for (int i = 0; i < kBlock / 64; ++i) s += red[i];
    if (s) atomicAdd(dst, s);
  }
}


// Streaming-policy store (NT kernels): write-through with sc1, so the once-written output does
// not leave dirty lines in the XCD's L2 (measured +3% over an nt store on the mix kernel at two
// workgroups per CU, tools/tune_cache_policy.py); the sequential mix's one-workgroup shape of long
// buckets stores nontemporally instead (kStoreNt, +1%, tools/probe/ab_store_r03.sh). Buffer
// stores take 32-bit offsets: the host splits a vector body into launches of at most kMaxChunkVec
// float4 (2 GiB).
constexpr long long kMaxChunkVec = 1LL << 27;
constexpr int kStoreSc1 = 16;
constexpr int kStoreNt = 2;

// The host side of that split: fn(done, m) for each chunk of m <= kMaxChunkVec float4 at `done`.
template <typename F>
inline void for_each_chunk(long long nvec, F&& fn) {
  for (long long done = 0; done < nvec; done += kMaxChunkVec)
    fn(done, (nvec - done) < kMaxChunkVec ? (nvec - done) : kMaxChunkVec);
}

// The streaming buffer store: the output resource of a chunk of `bytes` bytes (16 per float4, at
// most 2 GiB), and the store of 16-byte vector idx of it (a 32-bit byte offset) with a
// compile-time policy (kStoreSc1 / kStoreNt).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t out_rsrc(void* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(base, 0, bytes, 0x00020000);
}
template <int POLICY, typename V>
__device__ __forceinline__ void st16_buf(__amdgpu_buffer_rsrc_t r, long long idx, V v) {
  static_assert(sizeof(V) == 16, "16-byte vectors only");
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4v, v), r, (int)(idx * 16), 0, POLICY);
}

// Streaming store of one 16-byte vector with the sc1 write-through policy, as the headline mix
// stores its output (kStoreSc1), for outputs the host does not chunk: through the buffer store
// when every byte offset of the output fits the 31 bits the kernels pass, else a nontemporal
// global store. The choice is uniform per launch (one scalar branch).
struct Sc1Out {
  __amdgpu_buffer_rsrc_t r;
  void* base;
  bool buf;
};
__device__ __forceinline__ Sc1Out sc1_out(void* base, long long bytes) {
  Sc1Out o;
  o.base = base;
  o.buf = bytes <= 0x7FFFFFF0LL;
  o.r = out_rsrc(base, o.buf ? (unsigned)bytes : 0u);
  return o;
}
template <typename V>
__device__ __forceinline__ void st16_sc1(const Sc1Out& o, long long idx, V v) {  // idx: 16-byte units
  if (o.buf)
    st16_buf<kStoreSc1>(o.r, idx, v);
  else
    __builtin_nontemporal_store(v, reinterpret_cast<V*>(o.base) + idx);
}

// fp64 form of the epilogue for the fp64 chains (TF1 W_up_l2 is fp64 in the reference).
__device__ __forceinline__ double compress_one_d(double y, double ref, const CompressParams& cp,
                                                 unsigned& kept) {
  if (cp.mode == CFA_COMPRESS_SPARSE || cp.mode == CFA_COMPRESS_SPARSE_HI) {
    if (fabs(y) < cp.thr) return np_sign(y) * cp.rep;
  } else if (cp.mode == CFA_COMPRESS_SPARSE_DPCM || cp.mode == CFA_COMPRESS_SPARSE_DPCM_HI) {
    const double d = y - ref;
    if (fabs(d) < cp.thr) return ref + np_sign(d) * cp.rep;
  }
  ++kept;
  return y;
}

static inline uintptr_t addr(const void* p) { return reinterpret_cast<uintptr_t>(p); }

static int compress_params(int mode, CompressParams& cp) {
  cp.mode = mode;
  switch (mode) {
    case CFA_COMPRESS_NONE: cp.thr = 0.0; cp.rep = 0.0; break;
    case CFA_COMPRESS_SPARSE: cp.thr = 0.001; cp.rep = 0.0001; break;
    case CFA_COMPRESS_SPARSE_DPCM: cp.thr = 1.e-4; cp.rep = 1.e-4; break;
    case CFA_COMPRESS_SPARSE_DPCM_HI: cp.thr = 1.e-3; cp.rep = 1.e-3; break;
    case CFA_COMPRESS_SPARSE_HI: cp.thr = 0.01; cp.rep = 0.001; break;
    default: return fail(CFA_E_INVALID, "unknown compression mode %d", mode);
  }
  return CFA_OK;
}

static int validate_mix(const float* out, const float* local, const float* const* nbrs, int n,
                        size_t P) {
  if (n < 0) return fail(CFA_E_INVALID, "negative fan-in %d", n);
  if (P == 0) return CFA_OK;
  if (!out || !local) return fail(CFA_E_INVALID, "null out/local bucket");
  if (n > 0 && !nbrs) return fail(CFA_E_INVALID, "null neighbour table");
  for (int j = 0; j < n; ++j) {
    if (!nbrs[j]) return fail(CFA_E_INVALID, "null neighbour bucket %d", j);
    if (nbrs[j] == out) return fail(CFA_E_INVALID, "output aliases neighbour %d", j);
  }
  return CFA_OK;
}

static bool needs_ref(int mode) {
  return mode == CFA_COMPRESS_SPARSE_DPCM || mode == CFA_COMPRESS_SPARSE_DPCM_HI;
}

// ------------------------------------------------------------------------------------------
// Rounds of a device-resident population (cfa_population.hip, cfa_fedavg.hip).
// ------------------------------------------------------------------------------------------
// A schedule: round r works on table sched[r mod S] of T tables. The round counter is a device
// word, so a captured period of rounds replays with another table each time. Every workgroup of a
// round reads the same counter: advance_round raises it after the round, in stream order.
struct SchedArgs {
  const int32_t* sched;       // [S] table index of each slot
  unsigned long long* round;  // the round counter
  unsigned S;
};

// The table index of the current round: one chain of uniform loads (round -> sched).
__device__ __forceinline__ int sched_slot(const SchedArgs& sc) {
  const unsigned long long r = *static_cast<const unsigned long long*>(sc.round);
  return sc.sched[r % sc.S];
}

// The first entry of idx[b, e) whose device is flagged, e when there is none: the workgroup's
// lanes take one entry each per pass and keep the smallest flagged position. Called by every lane
// of the workgroup (it synchronises).
__device__ __forceinline__ int first_flagged(const int32_t* flags, const int32_t* idx, int b, int e) {
  __shared__ int first;
  if (threadIdx.x == 0) first = e;
  __syncthreads();
  for (int k = b + (int)threadIdx.x; k < e; k += kBlock)
    if (flags[idx[k]]) {
      atomicMin(&first, k);
      break;
    }
  __syncthreads();
  return __builtin_amdgcn_readfirstlane(first);
}

// A scheduled entry's own arguments, checked before anything else; sc.sched == nullptr stands for
// the static entry points' one table.
static int sched_args(const int32_t* sched, int S, int T, unsigned long long* round, SchedArgs& sc) {
  if (S <= 0 || T <= 0) return fail(CFA_E_INVALID, "schedule of %d slots over %d tables", S, T);
  if (!sched || !round) return fail(CFA_E_INVALID, "null schedule or round counter");
  sc = SchedArgs{sched, round, (unsigned)S};
  return CFA_OK;
}
// The round is over: the next launch on the stream reads the counter one higher.
static int advance_round(const SchedArgs& sc, hipStream_t st) { return advance_counter(sc.round, st); }
}  // namespace

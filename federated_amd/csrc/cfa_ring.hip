// cfa_ring.hip — the ring family of whole-population rounds: the sliding-window passes
// (cfa_mix_window_f32) that load each row of a ring window once for up to 8 consecutive devices,
// a whole ring-window round in one launch (cfa_mix_ring_round_f32), and the sliding ring round
// (cfa_mix_ring_slide_f32) that reads every row of a run of ring devices once. The step is
// seq_step of cfa_internal.h.
#include <type_traits>

#include "cfa_internal.h"
#include "cfa_slide_shape.h"

namespace {

// ------------------------------------------------------------------------------------------
// Sliding-window population pass (cfa_mix_window_f32): nb <= 8 consecutive devices of a ring
// window (hl below, hr above) share their rows, so each row of the window is loaded ONCE per
// element for all nb devices: (nb + hl + hr) reads + nb writes instead of nb * (hl + hr + 2).
// Device b's local row is rows[b + hl]; its neighbours, in the reference window's order
// (g-hl .. g-1, g+1 .. g+hr), are rows[b .. b+hl-1], rows[b+hl+1 .. b+hl+hr].
// ------------------------------------------------------------------------------------------
constexpr int kWinMaxDev = 8;
struct WindowArgs {
  const float* rows[kWinMaxDev + 8];
  float* out[kWinMaxDev];
  float a[kWinMaxDev];  // one coefficient per device, used for each of its steps
  int nb;
};

// The fold of one ring device over its window's HL + HR + 1 rows, row(j) = the j-th row of the
// window (the local row is row(HL)): the local row, then the rows below in ascending order, then
// the rows above, as the reference window's order.
template <int HL, int HR, typename Row>
__device__ __forceinline__ f4 ring_fold(Row row, float a) {
  f4 acc = row(HL);
#pragma unroll
  for (int j = 0; j < HL; ++j) acc = seq_step(acc, row(j), a);
#pragma unroll
  for (int j = 0; j < HR; ++j) acc = seq_step(acc, row(HL + 1 + j), a);
  return acc;
}

template <int HL, int HR, int U, bool SC1>
__device__ __forceinline__ void window_body(const WindowArgs& w, long long nvec) {
  constexpr int R = kWinMaxDev + HL + HR;
  constexpr long long kTile = (long long)kBlock * U;
  const int nr = w.nb + HL + HR;
  for (long long t = blockIdx.x; t * kTile < nvec; t += gridDim.x) {
    const long long base = t * kTile + threadIdx.x;
    f4 r[U][R];
#pragma unroll
    for (int k = 0; k < R; ++k)
      if (k < nr)
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const long long i = base + (long long)u * kBlock;
          if (i < nvec) r[u][k] = ld4<true>(w.rows[k], i);
        }
#pragma unroll
    for (int b = 0; b < kWinMaxDev; ++b)
      if (b < w.nb) {
        // (unused and removed by the compiler when !SC1) write-through streaming store
        const __amdgpu_buffer_rsrc_t o = out_rsrc(w.out[b], (unsigned)(nvec * 16));
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const long long i = base + (long long)u * kBlock;
          if (i < nvec) {
            const f4 y = ring_fold<HL, HR>([&](int j) { return r[u][b + j]; }, w.a[b]);
            if constexpr (SC1)
              st16_buf<kStoreSc1>(o, i, y);
            else
              st4<true>(w.out[b], i, y);
          }
        }
      }
  }
}

template <int HL, int HR, int U, bool SC1>
__global__ __launch_bounds__(kBlock) void window_vec_kernel(WindowArgs w, long long nvec) {
  window_body<HL, HR, U, SC1>(w, nvec);
}

// A whole ring-window round of a stacked population in ONE launch (cfa_mix_ring_round_f32):
// grid.y = pass p over devices [8p, 8p + nb); each block derives its pass's rows from the stack
// base and pitch (row g of the window = in + ((8p - HL + g) mod D) * pitch), then runs the
// window pass body. Same operations as one cfa_mix_window_f32 launch per pass.
struct RingArgs {
  const float* in;
  float* out;
  const float* alphas;  // [D] device array, one coefficient per device
  long long pitch;      // floats between consecutive devices' rows
  long long off;        // element offset of this launch's chunk
  int D;
};

template <int HL, int HR, int U, bool SC1>
__global__ __launch_bounds__(kBlock) void ring_round_kernel(RingArgs ra, long long nvec) {
  const int p = blockIdx.y;
  WindowArgs w;
  w.nb = min(kWinMaxDev, ra.D - p * kWinMaxDev);
#pragma unroll
  for (int k = 0; k < kWinMaxDev + HL + HR; ++k) {
    const int g = ((p * kWinMaxDev - HL + k) % ra.D + ra.D) % ra.D;
    w.rows[k] = ra.in + (long long)g * ra.pitch + ra.off;
  }
#pragma unroll
  for (int b = 0; b < kWinMaxDev; ++b) {
    const int d = min(p * kWinMaxDev + b, ra.D - 1);
    w.out[b] = ra.out + (long long)d * ra.pitch + ra.off;
    w.a[b] = ra.alphas[d];
  }
  window_body<HL, HR, U, SC1>(w, nvec);
}

// ------------------------------------------------------------------------------------------
// Sliding ring round (cfa_mix_ring_slide_f32): every row of a run of consecutive ring devices is
// read ONCE and every output written once. A workgroup owns a column tile of kBlock * U float4
// (lane x holds vectors base + v * kBlock, v < U, so each wave instruction is a contiguous 1 KB)
// and a segment (blockIdx.y) of `seg` consecutive devices. It walks the segment's row stream
// (rows d0-HL .. d0+len-1+HR, mod `rows`) through a ring of W + PF register slots of U float4,
// W = HL+HR+1: device m of the segment folds stream rows m .. m+W-1 (its local row is m+HL) while
// the loads of rows m+W .. m+W-1+PF are in flight. The device loop is unrolled W + PF times, so
// stream row q always sits in slot q mod (W + PF) and every register index is static. A segment
// re-reads HL+HR halo rows: a call of S segments reads count + S*K - (full ring ? K : 0) rows,
// K = HL+HR. The fold is the window pass's (ring_fold), on the slots the window's rows sit in, per
// vector.
//
// Seam rows once (SEAM, launched where slide_takes_seam allows): the stream of a full ring in one segment ends
// with the K rows it began with. While priming, a lane keeps a second copy of those rows' U
// vectors, the first K - slide_seam_lds_rows(K) in registers and the rest in LDS; the walk's last
// K "loads" take the copies and issue no global load. A lane reads back only what it wrote itself
// (vector (row * U + v) * kBlock + lane of the workgroup's LDS), so there is no barrier. Fold,
// operand order and stores are the plain walk's; PF is 1 and the stores nontemporal.
// ------------------------------------------------------------------------------------------
struct SlideArgs {
  const float* in;
  float* out;
  const float* alphas;             // [count] device array, one coefficient per device of the run
  long long in_pitch, out_pitch;   // floats between consecutive rows
  long long off;                   // element offset of this launch's chunk
  int rows, first, count, seg;     // seg: devices per segment
};

__device__ __forceinline__ f4* slide_seam_lds() {
  extern __shared__ __attribute__((aligned(16))) f4 seam_lds[];
  return seam_lds;
}

// SEAM is held to the occupancy of the plain kernel's tuned shapes (slide_seam_waves per SIMD).
template <int HL, int HR, int PF, int U, bool SC1, bool SEAM = false>
__global__ __launch_bounds__(kBlock, SEAM ? slide_seam_waves(U) : 1) void ring_slide_kernel(SlideArgs sa,
                                                                                            long long nvec) {
  constexpr int W = HL + HR + 1;
  constexpr int RS = W + PF;
  constexpr int K = HL + HR;                               // seam rows of a full ring
  constexpr int KV = SEAM ? K - slide_seam_lds_rows(K) : 0;  // of them, kept in registers
  constexpr long long kTile = (long long)kBlock * U;
  const int n0 = (int)blockIdx.y * sa.seg;  // first device of the segment, relative to sa.first
  const int len = min(sa.seg, sa.count - n0);
  const int total = len + HL + HR;  // rows of the segment's stream
  const int d0 = sa.first + n0;
  int g0 = (d0 - HL) % sa.rows;
  if (g0 < 0) g0 += sa.rows;
  const int o0 = d0 >= sa.rows ? d0 - sa.rows : d0;
  const float* const in = sa.in + sa.off;
  float* const out = sa.out + sa.off;
  const float* const in_end = in + (long long)sa.rows * sa.in_pitch;
  float* const out_end = out + (long long)sa.rows * sa.out_pitch;
  for (long long t = blockIdx.x; t * kTile < nvec; t += gridDim.x) {
    const long long i = t * kTile + threadIdx.x;
    if (i >= nvec) continue;  // the stripes ascend: a lane without its first vector has none
    // Byte offsets of the lane's vectors (a chunk is at most kMaxChunkVec float4: below 2^31). In
    // the last tile a stripe may lie partly or wholly past nvec: such a vector loads the lane's
    // first vector again (in bounds, so the loads need no branch) and is never stored.
    bool ok[U];
    unsigned voff[U];
#pragma unroll
    for (int v = 0; v < U; ++v) {
      ok[v] = i + (long long)v * kBlock < nvec;
      voff[v] = (unsigned)((ok[v] ? i + (long long)v * kBlock : i) * 16);
    }
    const float* rp = in + (long long)g0 * sa.in_pitch;  // next row of the stream to load
    float* op = out + (long long)o0 * sa.out_pitch;      // next output row
    f4 r[RS][U];
    auto load_row = [&](f4(&slot)[U]) {  // all U loads of the stream's next row
#pragma unroll
      for (int v = 0; v < U; ++v)
        slot[v] = __builtin_nontemporal_load(reinterpret_cast<const f4*>(reinterpret_cast<const char*>(rp) + voff[v]));
      rp += sa.in_pitch;
      if (rp == in_end) rp = in;
    };
#pragma unroll
    for (int q = 0; q < RS - 1; ++q)
      if (q < total) load_row(r[q]);
    // SEAM: the lane's second copy of stream rows 0 .. K-1 (all primed above: total > RS - 1 > K on
    // a full ring), the first KV in registers and the rest in the lane's own LDS vectors.
    [[maybe_unused]] f4 keep[KV > 0 ? KV : 1][U];
    if constexpr (SEAM) {
#pragma unroll
      for (int q = 0; q < K; ++q)
#pragma unroll
        for (int v = 0; v < U; ++v) {
          if (q < KV) keep[q][v] = r[q][v];
          else slide_seam_lds()[((q - KV) * U + v) * kBlock + threadIdx.x] = r[q][v];
        }
    }
    for (int n = 0; n < len; n += RS) {
#pragma unroll
      for (int u = 0; u < RS; ++u) {
        const int m = n + u;
        if (m < len) {
          // stream row m+W-1+PF: into the slot row m-1 has left
          if constexpr (SEAM) {
            // rows len .. len+K-1 of a full ring's stream are its rows 0 .. K-1 again
            if (m + RS - 1 >= len) {
              const int j = m + RS - 1 - len;  // retained row j instead of its loads
              f4(&slot)[U] = r[(u + RS - 1) % RS];
              if (j >= K) {  // past the stream's end
              } else if (j >= KV) {
#pragma unroll
                for (int v = 0; v < U; ++v) slot[v] = slide_seam_lds()[((j - KV) * U + v) * kBlock + threadIdx.x];
              } else {
#pragma unroll
                for (int k = 0; k < KV; ++k)  // uniform branches: every register index static
                  if (j == k)
#pragma unroll
                    for (int v = 0; v < U; ++v) slot[v] = keep[k][v];
              }
            } else {
              load_row(r[(u + RS - 1) % RS]);
            }
          } else {
            if (m + RS - 1 < total) load_row(r[(u + RS - 1) % RS]);
          }
          const float a = sa.alphas[n0 + m];
          f4 acc[U];
#pragma unroll
          for (int v = 0; v < U; ++v) acc[v] = ring_fold<HL, HR>([&](int j) { return r[(u + j) % RS][v]; }, a);
#pragma unroll
          for (int v = 0; v < U; ++v)
            if (ok[v]) {
              if constexpr (SC1)
                st16_buf<kStoreSc1>(out_rsrc(op, (unsigned)(nvec * 16)), i + (long long)v * kBlock, acc[v]);
              else
                __builtin_nontemporal_store(acc[v], reinterpret_cast<f4*>(reinterpret_cast<char*>(op) + voff[v]));
            }
          op += sa.out_pitch;
          if (op == out_end) op = out;
        }
      }
    }
  }
}

// Scalar window pass (misaligned rows, the < 4-element tail): runtime hl / hr.
__global__ __launch_bounds__(kBlock) void window_scalar_kernel(WindowArgs w, int hl, int hr,
                                                               long long begin, long long P) {
  for (long long i = begin + (long long)blockIdx.x * kBlock + threadIdx.x; i < P;
       i += (long long)gridDim.x * kBlock) {
    for (int b = 0; b < w.nb; ++b) {
      float acc = w.rows[b + hl][i];
      for (int j = 0; j < hl; ++j) acc = seq_step(acc, w.rows[b + j][i], w.a[b]);
      for (int j = 0; j < hr; ++j) acc = seq_step(acc, w.rows[b + hl + 1 + j][i], w.a[b]);
      w.out[b][i] = acc;
    }
  }
}

}  // namespace

namespace {
struct WindowTune {
  int vec, sc1, blocks_per_cu;
};
static WindowTune window_tune() {  // env overrides for tools/tune_window.py; results identical
  WindowTune t{1, 0, 6};  // tools/tune_window.py, profiles/r01_tune_window.jsonl
  t.vec = env_int("CFA_WINDOW_VEC", t.vec) == 1 ? 1 : 2;
  t.sc1 = env_int("CFA_WINDOW_SC1", t.sc1) ? 1 : 0;
  t.blocks_per_cu = env_int("CFA_WINDOW_BLOCKS_PER_CU", t.blocks_per_cu);
  if (t.blocks_per_cu <= 0) t.blocks_per_cu = 2;  // kept as it is: not the default 6
  return t;
}
static long long window_tiles(long long m, const WindowTune& t) {
  return (m + (long long)kBlock * t.vec - 1) / ((long long)kBlock * t.vec);
}
// The run-time (vec, sc1) of a window launch as the kernels' <U, SC1>: fn(U, SC1) gets them as
// std::integral_constant values.
template <typename F>
void for_vec_sc1(const WindowTune& t, F&& fn) {
  using One = std::integral_constant<int, 1>;
  using Two = std::integral_constant<int, 2>;
  if (t.vec == 1) {
    if (t.sc1) fn(One{}, std::true_type{});
    else fn(One{}, std::false_type{});
  } else {
    if (t.sc1) fn(Two{}, std::true_type{});
    else fn(Two{}, std::false_type{});
  }
}
template <int HL, int HR>
void launch_window(const WindowArgs& w, long long nvec, hipStream_t st) {
  const WindowTune t = window_tune();
  const cfa_launch_t lc{t.blocks_per_cu, t.vec, 1};
  for_each_chunk(nvec, [&](long long done, long long m) {
    WindowArgs c = w;
    for (int k = 0; k < w.nb + HL + HR; ++k) c.rows[k] = w.rows[k] + done * 4;
    for (int b = 0; b < w.nb; ++b) c.out[b] = w.out[b] + done * 4;
    const unsigned grid = grid_for(window_tiles(m, t), lc);
    for_vec_sc1(t, [&](auto u, auto sc1) {
      window_vec_kernel<HL, HR, decltype(u)::value, decltype(sc1)::value><<<grid, kBlock, 0, st>>>(c, m);
    });
  });
}
template <int HL, int HR>
void launch_ring_round(const RingArgs& ra, long long nvec, hipStream_t st) {
  const WindowTune t = window_tune();
  const cfa_launch_t lc{t.blocks_per_cu, t.vec, 1};
  const unsigned passes = (unsigned)((ra.D + kWinMaxDev - 1) / kWinMaxDev);
  for_each_chunk(nvec, [&](long long done, long long m) {
    RingArgs c = ra;
    c.off = ra.off + done * 4;
    const long long tiles = window_tiles(m, t);
    // the launch's blocks over all passes: about blocks_per_cu per CU in all. Not shared_grid_x:
    // the tiles are capped before the division by the passes (10 tiles over 16 passes give 1, not 10)
    long long gx = (grid_for(tiles, lc) + passes - 1) / passes;
    if (gx < 1) gx = 1;
    if (gx > tiles) gx = tiles;
    const dim3 grid((unsigned)gx, passes);
    for_vec_sc1(t, [&](auto u, auto sc1) {
      ring_round_kernel<HL, HR, decltype(u)::value, decltype(sc1)::value><<<grid, kBlock, 0, st>>>(c, m);
    });
  });
}

// Launch shape of the sliding ring round. The environment overrides are read at each launch, so
// one process can compare shapes on the same buffers (tools/probe/ring_slide.py); results are
// identical for every shape. SlideTune and its default are in cfa_slide_shape.h; here u = 0 stands
// for the tuned width, stepped down where a short row would leave workgroups without a tile
// (slide_pick_u), and CFA_SLIDE_U = 1, 2 or 4 for exactly that width. CFA_SLIDE_SEAM = 0 keeps a
// full ring on the plain kernel, 1 sends it to the seam kernel where slide_takes_seam allows
// (nontemporal stores only; the seam kernel's PF is 1 whatever CFA_SLIDE_PF says).
static_assert(kSlideBlock == kBlock, "cfa_slide_shape.h counts tiles of kBlock lanes");
static SlideTune slide_tune() {
  const SlideTune d = kSlideDefault;
  SlideTune t{env_int("CFA_SLIDE_SEGMENTS", d.segments), env_int("CFA_SLIDE_WG_PER_CU", d.wg_per_cu),
              env_int("CFA_SLIDE_PF", d.pf), env_int("CFA_SLIDE_SC1", d.sc1) ? 1 : 0, env_int("CFA_SLIDE_U", 0)};
  if (t.segments <= 0) t.segments = d.segments;
  if (t.wg_per_cu <= 0) t.wg_per_cu = d.wg_per_cu;
  if (t.pf < 1 || t.pf > 2) t.pf = d.pf;
  if (t.u != 1 && t.u != 2 && t.u != 4) t.u = 0;
  return t;
}
template <int HL, int HR, int PF, int U>
void launch_slide_shape(const SlideArgs& c, long long m, dim3 grid, bool sc1, hipStream_t st) {
  if (sc1) ring_slide_kernel<HL, HR, PF, U, true><<<grid, kBlock, 0, st>>>(c, m);
  else ring_slide_kernel<HL, HR, PF, U, false><<<grid, kBlock, 0, st>>>(c, m);
}
template <int HL, int HR, int U>
void launch_slide_u(const SlideArgs& c, long long m, dim3 grid, const SlideTune& t, hipStream_t st) {
  switch (t.pf) {
    case 1: launch_slide_shape<HL, HR, 1, U>(c, m, grid, t.sc1, st); break;
    default: launch_slide_shape<HL, HR, 2, U>(c, m, grid, t.sc1, st); break;
  }
}
// The seam kernel of a full ring in one segment; false (nothing launched) where the window retains
// nothing or the device refuses the kernel its LDS. Above 64 KB the kernel's dynamic-LDS limit is
// raised first, once per device (as cfa_grad.hip's kernels).
template <int HL, int HR, int U>
bool slide_seam_lds_ready() {
  constexpr int bytes = slide_seam_lds_bytes(HL + HR, U);
  if constexpr (bytes > 65536) {
    static unsigned long long raised = 0;  // bit per device
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    if (__atomic_load_n(&raised, __ATOMIC_RELAXED) >> dev & 1) return true;
    if (bytes > device_lds_max() ||
        hipFuncSetAttribute(reinterpret_cast<const void*>(&ring_slide_kernel<HL, HR, 1, U, false, true>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    __atomic_fetch_or(&raised, 1ULL << dev, __ATOMIC_RELAXED);
  }
  return true;
}
template <int HL, int HR, int U>
bool launch_slide_seam(const SlideArgs& c, long long m, dim3 grid, hipStream_t st) {
  if constexpr (HL + HR >= 1) {
    if (!slide_seam_lds_ready<HL, HR, U>()) return false;
    ring_slide_kernel<HL, HR, 1, U, false, true><<<grid, kBlock, slide_seam_lds_bytes(HL + HR, U), st>>>(c, m);
    return true;
  } else {
    return false;
  }
}
template <int HL, int HR>
void launch_ring_slide(const SlideArgs& sa, long long nvec, hipStream_t st) {
  const SlideTune t = slide_tune();
  const bool seam_wanted = env_int("CFA_SLIDE_SEAM", kSlideSeamDefault) != 0 && !t.sc1;
  int segments = t.segments < sa.count ? t.segments : sa.count;
  if (segments > 65535) segments = 65535;
  SlideArgs c = sa;
  c.seg = (sa.count + segments - 1) / segments;
  const unsigned gy = (unsigned)((sa.count + c.seg - 1) / c.seg);  // no empty segment
  for_each_chunk(nvec, [&](long long done, long long m) {
    c.off = done * 4;
    const int u = t.u ? t.u : slide_pick_u(m, kSlideDefault.u, device_cus(), t.wg_per_cu);
    // the launch's workgroups over all segments: about wg_per_cu per CU in all
    const dim3 grid(shared_grid_x(slide_tiles(m, u), t.wg_per_cu, gy), gy);
    if (seam_wanted && slide_takes_seam(sa.rows, sa.count, (int)gy, HL, HR, u) &&
        (u == 4 ? launch_slide_seam<HL, HR, 4>(c, m, grid, st) : launch_slide_seam<HL, HR, 2>(c, m, grid, st)))
      return;
    switch (u) {
      case 4: launch_slide_u<HL, HR, 4>(c, m, grid, t, st); break;
      case 2: launch_slide_u<HL, HR, 2>(c, m, grid, t, st); break;
      default: launch_slide_u<HL, HR, 1>(c, m, grid, t, st); break;
    }
  });
}

// The launchers by (hl, hr), each 0..4: the one definition of the 5x5 table.
#define CFA_HLHR_ROW(F, L) {&F<L, 0>, &F<L, 1>, &F<L, 2>, &F<L, 3>, &F<L, 4>}
#define CFA_HLHR_TABLE(F) \
  {CFA_HLHR_ROW(F, 0), CFA_HLHR_ROW(F, 1), CFA_HLHR_ROW(F, 2), CFA_HLHR_ROW(F, 3), CFA_HLHR_ROW(F, 4)}
void (*const kWindowLaunch[5][5])(const WindowArgs&, long long, hipStream_t) = CFA_HLHR_TABLE(launch_window);
void (*const kRingLaunch[5][5])(const RingArgs&, long long, hipStream_t) = CFA_HLHR_TABLE(launch_ring_round);
void (*const kSlideLaunch[5][5])(const SlideArgs&, long long, hipStream_t) = CFA_HLHR_TABLE(launch_ring_slide);
template <int HL, int HR>
void slide_seam_prepare() {
  if constexpr (HL + HR >= 1) (void)(slide_seam_lds_ready<HL, HR, 4>() && slide_seam_lds_ready<HL, HR, 2>());
}
void (*const kSlideSeamPrepare[5][5])() = CFA_HLHR_TABLE(slide_seam_prepare);
#undef CFA_HLHR_TABLE
#undef CFA_HLHR_ROW
}  // namespace

// Current device: raise the seam kernels' dynamic-LDS limit now (cfa_device_prepare), so later
// launches (e.g. under hipGraph capture) need no attribute call. Refused: those windows' full
// rings stay on the plain kernel.
int ring_prepare_device() {
  for (int hl = 0; hl <= 4; ++hl)
    for (int hr = 0; hr <= 4; ++hr) kSlideSeamPrepare[hl][hr]();
  return CFA_OK;
}

extern "C" int cfa_mix_window_f32(float* const* out, const float* const* rows, const float* alphas,
                                  int nb, int hl, int hr, size_t P, void* stream) {
  if (nb < 1 || nb > kWinMaxDev) return fail(CFA_E_INVALID, "nb %d outside 1..%d", nb, kWinMaxDev);
  if (hl < 0 || hr < 0 || hl > 4 || hr > 4) return fail(CFA_E_INVALID, "window %d/%d outside 0..4", hl, hr);
  if (!out || !rows || !alphas) return fail(CFA_E_INVALID, "null table");
  if (P == 0) return CFA_OK;
  WindowArgs w{};
  w.nb = nb;
  const int nr = nb + hl + hr;
  bool aligned = true;
  for (int k = 0; k < nr; ++k) {
    if (!rows[k]) return fail(CFA_E_INVALID, "null row %d", k);
    w.rows[k] = rows[k];
    aligned = aligned && (addr(rows[k]) & 15) == 0;
  }
  for (int b = 0; b < nb; ++b) {
    if (!out[b]) return fail(CFA_E_INVALID, "null output %d", b);
    for (int k = 0; k < nr; ++k)
      if (out[b] == rows[k]) return fail(CFA_E_INVALID, "output %d aliases row %d", b, k);
    w.out[b] = out[b];
    aligned = aligned && (addr(out[b]) & 15) == 0;
    w.a[b] = alphas[b];
  }
  hipStream_t st = (hipStream_t)stream;
  const long long nvec = aligned ? (long long)(P / 4) : 0;
  if (nvec > 0) {
    kWindowLaunch[hl][hr](w, nvec, st);
    if (int rc = check_launch("window_vec")) return rc;
  }
  const long long begin = nvec * 4;
  if (begin < (long long)P) {
    const long long len = (long long)P - begin;
    window_scalar_kernel<<<grid_for((len + kBlock - 1) / kBlock), kBlock, 0, st>>>(w, hl, hr, begin, (long long)P);
    if (int rc = check_launch("window_scalar")) return rc;
  }
  return CFA_OK;
}

extern "C" int cfa_mix_ring_round_f32(float* out, const float* in, size_t pitch, const float* alphas, int D,
                                      int hl, int hr, size_t P, void* stream) {
  if (D < 1) return fail(CFA_E_INVALID, "device count %d", D);
  if (hl < 0 || hr < 0 || hl > 4 || hr > 4) return fail(CFA_E_INVALID, "window %d/%d outside 0..4", hl, hr);
  if (hl + hr >= D) return fail(CFA_E_INVALID, "window %d/%d wider than %d devices", hl, hr, D);
  if (!out || !in || !alphas) return fail(CFA_E_INVALID, "null buffer");
  if (pitch < P) return fail(CFA_E_INVALID, "pitch %zu below P %zu", pitch, P);
  if (P == 0) return CFA_OK;
  if ((addr(out) & 15) || (addr(in) & 15) || (pitch % 4) || (P % 4))
    return fail(CFA_E_UNSUPPORTED, "ring round needs 16-byte aligned rows (pitch and P multiples of 4)");
  const long long outb = (long long)addr(out), inb = (long long)addr(in), span = (long long)D * (long long)pitch * 4;
  if (outb < inb + span && inb < outb + span) return fail(CFA_E_INVALID, "out overlaps in");
  if ((long long)(D + kWinMaxDev - 1) / kWinMaxDev > 65535) return fail(CFA_E_INVALID, "D=%d exceeds grid.y", D);
  RingArgs ra{in, out, alphas, (long long)pitch, 0, D};
  kRingLaunch[hl][hr](ra, (long long)(P / 4), (hipStream_t)stream);
  return check_launch("ring_round");
}

extern "C" int cfa_mix_ring_slide_f32(float* out, size_t out_pitch, const float* in, size_t in_pitch,
                                      const float* alphas, int rows, int first, int count, int hl, int hr,
                                      size_t P, void* stream) {
  if (!out || !in || !alphas) return fail(CFA_E_INVALID, "null buffer");
  if (rows < 1 || count < 1) return fail(CFA_E_INVALID, "rows %d / count %d below 1", rows, count);
  if (first < 0 || first >= rows || count > rows || (count != rows && first > rows - count))
    return fail(CFA_E_INVALID, "devices %d..%d outside a ring of %d rows", first, first + count - 1, rows);
  if (hl < 0 || hr < 0 || hl > 4 || hr > 4) return fail(CFA_E_INVALID, "window %d/%d outside 0..4", hl, hr);
  if (hl + hr >= rows) return fail(CFA_E_INVALID, "window %d/%d wider than %d rows", hl, hr, rows);
  if (in_pitch < P || out_pitch < P)
    return fail(CFA_E_INVALID, "pitch %zu/%zu below P %zu", out_pitch, in_pitch, P);
  if (P == 0) return CFA_OK;
  const unsigned long long outb = addr(out), inb = addr(in);
  const unsigned long long out_span = ((unsigned long long)(rows - 1) * out_pitch + P) * 4;
  const unsigned long long in_span = ((unsigned long long)(rows - 1) * in_pitch + P) * 4;
  if (outb < inb + in_span && inb < outb + out_span) return fail(CFA_E_INVALID, "out overlaps in");
  if ((outb & 15) || (inb & 15) || (out_pitch % 4) || (in_pitch % 4) || (P % 4))
    return fail(CFA_E_UNSUPPORTED, "ring slide needs 16-byte aligned rows (pitches and P multiples of 4)");
  SlideArgs sa{in, out, alphas, (long long)in_pitch, (long long)out_pitch, 0, rows, first, count, count};
  kSlideLaunch[hl][hr](sa, (long long)(P / 4), (hipStream_t)stream);
  return check_launch("ring_slide");
}

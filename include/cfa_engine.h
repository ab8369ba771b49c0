/*
 * cfa_engine.h — C-ABI of libcfa.so, the MI355X (gfx950) consensus-reduction engine.
 *
 * This is the drop-in boundary for the CFA / CFA-GE neighbour-model mixing step of
 * labRadioVision/federated. The reference computes that step with numpy AXPY chains
 * inside its `consensus` package. Each entry point below replaces one of those chains
 * (citations are `path:line` under the reference tree; TF1 = tensorflow1_implementations,
 * TF2 = tensorflow2_implementations/MNIST_dataset unless stated).
 * The blocks marked (f3/f4) and (TF2 drivers) cover what a driver does on every device between
 * two mixing steps: the TF1 local SGD epoch, the TF2 optimizer step, the TF2 validation pass (the
 * forward pass of the LeNet-1 family and the training_end flag) and that family's minibatch gradient.
 *
 * Conventions
 *   - Plain pointers and sizes only. Buffers are caller-owned device pointers
 *     (hipMalloc / PyTorch-ROCm tensors). The library allocates no device memory on the hot
 *     path (scratch comes from the caller, e.g. the gradient workspace; the one exception is
 *     cfa_mix_tf1_f32 above CFA_MAX_FANIN neighbours, documented there, whose caller-scratch
 *     form is cfa_mix_tf1_ex_f32). The host-only MQTT
 *     payload codec allocates its parse tree in host memory (freed by cfa_payload_free).
 *   - `stream` is a hipStream_t passed as void*; NULL means the legacy default stream.
 *     Every compute call is asynchronous on that stream. Every device pointer of a call must be
 *     memory of the stream's GPU: the library does not query pointer attributes on the launch
 *     path, so another GPU's pointer is not refused here (the Python engine refuses such
 *     tensors, federated_amd/engine.py _same_device).
 *   - Return 0 on success, a negative CFA_E* code on failure. `cfa_last_error()` returns a
 *     thread-local message for the last failure on the calling thread. No exceptions cross
 *     the ABI. Calls are re-entrant and thread-safe. The one piece of process-wide state is the
 *     host copy pool behind the host mix entry below, whose workers are created on first use and
 *     never destroyed: one call owns it at a time, and a concurrent call copies on its own thread.
 *   - `P` is the bucket length in fp32 elements. A "bucket" is one model (or gradient)
 *     flattened layer by layer, in the order the reference passes its tensors.
 *   - Pointer arrays (`nbrs`, `alphas`, `coeff`, `s`, `g`) are HOST arrays whose entries are
 *     device pointers (or host scalars for coefficients).
 *   - `out` may alias `local` / `W` (in-place update). Outputs must not alias any neighbour.
 *   - Any fan-in n >= 0 is accepted; n > CFA_MAX_FANIN is executed as several passes.
 *   - hipGraph capture: call cfa_device_prepare(device) once per device before capturing. After
 *     it, no entry point issues a device-attribute query, a kernel-attribute change or an
 *     allocation on the launch path (cfa_mix_tf1_f32 above CFA_MAX_FANIN refuses capture and
 *     points to cfa_mix_tf1_ex_f32), so captures run in the strict (global) mode.
 *
 * Where the ABI departs from the signatures sketched in SURVEY.md §8(b), entry by entry
 * (tests/test_capi.py holds the sketch's parameter lists and checks every prototype below
 * against this list)
 *   - cfa_mix_f32(out, local, nbrs, coeff, n, P, stream): `coeff` and `n` are SWAPPED relative to
 *     the sketch's (out, local, nbrs, n, coeff, P, stream), so that every mix entry reads
 *     (out, local, nbrs, <per-neighbour host array>, n, P, ...) alike: cfa_mix_seq_f32 and
 *     cfa_mix_seq_div_f32 take alphas (and divisors) in that same slot. A C caller following the
 *     sketch must swap the two. The sequential rule is its own entry (alphas, not closed-form
 *     coefficients) because the reference's fp32 chain is three roundings per step, which no
 *     coefficient vector reproduces.
 *   - cfa_mewma_update_f32(W, s, g, g_stride, n, rho, lr1, lr2, lr_split, init, use_filtered, P,
 *     stream) against the sketch's (W, s, g, n, rho, lr, use_filtered, P, stream):
 *     `g_stride` (per-neighbour element stride of g_j, NULL = contiguous) reads the
 *     `[..., devices]` gradient slices the sketch gave to cfa_mix_strided_f32; `rho` is a double
 *     so rho and 1 - rho each round once to fp32 as numpy does with a Python float; the one `lr`
 *     becomes (lr1, lr2, lr_split) because the reference applies -l1 to the layer-1 tensors and
 *     -l2 to the layer-2 tensors of one bucket (federated_sample_CNN_CFA-GE.py:16-17,29-30);
 *     `init` selects the 4-stage epoch-1 rule s_j <- g_j (cfa_ge_2stage.py:332-336).
 *   - cfa_compress_epilogue_f32(y, ref, mode, P, kept_count, stream) against the sketch's
 *     (y, ref_or_null, thr, rep, mode, kept_count, P, stream): `mode` replaces (thr, rep), since
 *     the four (thr, rep) pairs are fixed by cfa_ongraphs.py:225-273 and the mode also selects the
 *     sparse vs DPCM test, which (thr, rep) alone cannot express (a mode makes an inconsistent
 *     triple unrepresentable); `P` comes before `kept_count`, the order of every sized entry here.
 *   - cfa_mix_population_f32(out_ptrs, src_ptrs, csr_ptr, csr_idx, csr_coef, D, rule, P, stream)
 *     against (out_stack, in_stack, csr_ptr, csr_idx, csr_coeff, D, P, stream): device tables of
 *     bucket pointers instead of dense stacks, because a population's devices live in separate
 *     buffers (ping-pong models, halo rows, per-device allocations from callers) and a pointer
 *     table serves all of them with one launch (a dense [D, P] stack is the special case,
 *     cfa_mix_ring_round_f32); `rule` added so one launch serves the sequential CFA rule and the
 *     linear FedAvg form.
 *   - cfa_comm_init(comm, rank, nranks, id, device) against (rank, nranks, id, comm): the
 *     communicator out parameter comes first and `device` is added, so a caller thread need not
 *     have selected the GPU beforehand; the return value stays the status code.
 *   - cfa_mix_strided_f32 is not provided. The `[..., devices]` gradient slices of CFA-GE
 *     (cfa_ge_2stage.py:594-606) arrive in host memory (loadmat), and the host mixer gathers slot
 *     `ii` while packing the pinned staging rows, so every GPU read is a coalesced row. Read on
 *     the device, a stride-D slice pulls a whole line per 4 useful bytes: the round-1 entry ran at
 *     0.31 of peak with 2.5x over-fetch, so it was retired in round 2 (g_stride above keeps the
 *     strided read for the MEWMA update, whose caller may hold such slices on the device).
 *   - cfa_halo_exchange_f32, whose parameters the sketch elides, takes whole buckets; it is joined by
 *     cfa_p2p_group_f32, with per-message counts, for the routed, chunked halo.
 *     cfa_allreduce_scaled_f32 became cfa_allreduce_sum_f32 / cfa_reduce_sum_f32 because the
 *     pre-scaling is fused into the mix that produces the buffer (one pass fewer).
 *   - cfa_comm_destroy, cfa_last_error and cfa_version are as sketched.
 */
#ifndef CFA_ENGINE_H
#define CFA_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define CFA_API __attribute__((visibility("default")))
#else
#define CFA_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define CFA_VERSION 10000 /* 1.0.0 */
#define CFA_MAX_FANIN 16  /* neighbours folded per kernel pass */

enum {
  CFA_OK = 0,
  CFA_E_INVALID = -1,     /* bad argument (null pointer, negative size, bad mode) */
  CFA_E_HIP = -2,         /* HIP runtime error (launch, memcpy, device) */
  CFA_E_RCCL = -3,        /* RCCL error */
  CFA_E_UNSUPPORTED = -4, /* feature not available in this build */
  CFA_E_TIMEOUT = -5      /* a host-side wait gave up (cfa_host_wait_word) */
};

/* Mixing rules. */
enum {
  /* Sequential CFA rule: w <- w + a_j * (x_j - w), j = 0..n-1, evaluated as
   * t = x_j - w; t = a_j * t; w = w + t (three fp32 roundings, no FMA contraction).
   * This reproduces the fp32 numpy chain bit for bit. */
  CFA_RULE_SEQUENTIAL = 0,
  /* Linear combination: out = c_0 * local + sum_j c_{j+1} * x_j (fp32 FMA chain). */
  CFA_RULE_LINEAR = 1,
  /* Sequential rule with a divisor: w <- w + (a_j * (x_j - w)) / d_j (FedAvg form). */
  CFA_RULE_SEQUENTIAL_DIV = 2,
  /* Accumulation: w <- w + a_j * x_j, one rounding per product and per sum (fp64 fold only). */
  CFA_RULE_ACCUMULATE = 3
};

/* Compression epilogue modes (TF1/consensus/cfa_ongraphs.py:225-273). The fp32 entry points
 * (cfa_mix_seq_compress_f32, cfa_compress_epilogue_f32) evaluate them as numpy 2 does on fp32
 * arrays: threshold and replacement cast to fp32, test / product / DPCM sum in fp32. The TF1
 * entry points (cfa_mix_tf1_f32, cfa_mix_tf1_f64) evaluate them in fp64 on the fp64 chain, as
 * the reference does on its promoted W_up_l2. */
enum {
  CFA_COMPRESS_NONE = 0,
  CFA_COMPRESS_SPARSE = 1,          /* |y| < 1e-3 -> sign(y) * 1e-4                       :227-237 */
  CFA_COMPRESS_SPARSE_DPCM = 2,     /* |y - ref| < 1e-4 -> ref + sign(y - ref) * 1e-4      :239-249 */
  CFA_COMPRESS_SPARSE_DPCM_HI = 3,  /* |y - ref| < 1e-3 -> ref + sign(y - ref) * 1e-3      :250-260 */
  CFA_COMPRESS_SPARSE_HI = 4        /* |y| < 1e-2 -> sign(y) * 1e-3                        :261-271 */
};

/* Client rules of the FedAvg population round (cfa_fedavg_population_round_f32). */
enum {
  CFA_CLIENT_NONE = 0, /* only the global model is written */
  CFA_CLIENT_COPY = 1, /* every device takes the global model as it is */
  CFA_CLIENT_MIX = 2   /* every device mixes it in: w <- w + (u_c * (g - w)) / d_c */
};

/* Modes of the TF1 CFA-FA server epoch (cfa_fa_population_round_f32). */
enum {
  CFA_FA_INIT = 0, /* epoch 0: s <- s + b_d * x_d, the devices keep their models */
  CFA_FA_ROUND = 1 /* later: s <- s + (eps * b_d) * (x_d - s), then W <- W + eps2 * (s - W) */
};

/* What a device does with the first neighbour that reports training_end
 * (cfa_mix_population_ended_f32). */
enum {
  CFA_ENDED_COPY = 0,        /* takes that neighbour's model as it is          consensus_v3.py:147-152 */
  CFA_ENDED_TRUNCATE = 1,    /* mixes the collected prefix, the table's eps    consensus_v4.py:234-248 */
  CFA_ENDED_TRUNCATE_EPS = 2 /* mixes it with eps = 1 / (prefix length + 1)    consensus_v3.py:233 */
};

/* Update rules of the population optimizer step (cfa_optim_step_f32). */
enum {
  CFA_OPTIM_SGD = 0,      /* w <- w - lr * g                                     SGD(learning_rate) */
  CFA_OPTIM_MOMENTUM = 1, /* a <- momentum * a - lr * g; w <- w + a              SGD(learning_rate, momentum) */
  CFA_OPTIM_ADAM = 2      /* Keras Adam without amsgrad, tf.clip_by_norm per layer first   Adam(learning_rate, clipnorm) */
};

/* The objective of the TF2 LeNet-1 kernels (cfa_lenet_eval_loss_f32, cfa_lenet_grad_loss_f32). */
enum {
  CFA_LENET_LOSS_XENT = 0, /* -log softmax(z)[label]                 ..._MNIST_crossentropy_gradients_exchange.py:321-337 */
  CFA_LENET_LOSS_HUBER = 1 /* Huber(label, softmax(z)[label])        federated_learning_keras_consensus_FL_MNIST.py:369-377 */
};

CFA_API int cfa_version(void);
CFA_API const char* cfa_last_error(void);

/* Caches `device`'s CU count and LDS size and raises the gradient kernels' dynamic-LDS limit on
 * it, so that later launches query nothing (required before a strict hipGraph capture). The
 * calling thread's current device is restored. Idempotent. */
CFA_API int cfa_device_prepare(int device);

/* ---------------------------------------------------------------------------------------
 * (f2) MATLAB level-5 files of the TF1 exchange (host only). Every TF1 consensus call publishes
 * its model with scipy.io.savemat and loads its neighbours' with scipy.io.loadmat
 * (TF1/consensus/cfa.py:108-117, 131-139; cfa_ongraphs.py:214-223, 282-291;
 * cfa_ge_2stage.py:537-606). cfa_mat_write writes the bytes scipy's level-5 writer writes for real
 * numeric matrices (uncompressed, column-major data, 8-byte padding, small-data elements at <= 4
 * bytes); cfa_mat_read parses such files (scipy's or MATLAB's, uncompressed, little-endian,
 * real numeric classes only) and returns CFA_E_UNSUPPORTED for anything else, so the caller can
 * fall back to scipy. The parsed file owns the memory its variables point into.
 */
#define CFA_MAT_MAX_DIM 8
typedef struct {
  const char* name;
  int mat_class;   /* mxDOUBLE_CLASS = 6, SINGLE 7, INT8 8, UINT8 9, INT16 10, UINT16 11, INT32 12,
                      UINT32 13, INT64 14, UINT64 15 */
  int mi_type;     /* stored element type: miINT8 1, miUINT8 2, miINT16 3, miUINT16 4, miINT32 5,
                      miUINT32 6, miSINGLE 7, miDOUBLE 9, miINT64 12, miUINT64 13 */
  int ndim;
  int64_t dims[CFA_MAT_MAX_DIM];
  const void* data; /* column-major elements of mi_type */
  size_t nbytes;
} cfa_mat_var_t;
typedef struct cfa_mat cfa_mat_t;
CFA_API int cfa_mat_read(const char* path, cfa_mat_t** out);
CFA_API void cfa_mat_free(cfa_mat_t* mat);
CFA_API int cfa_mat_num_vars(const cfa_mat_t* mat);
CFA_API const cfa_mat_var_t* cfa_mat_vars(const cfa_mat_t* mat);
CFA_API const char* cfa_mat_header(const cfa_mat_t* mat);
CFA_API int cfa_mat_write(const char* path, const char* header, int nvars, const cfa_mat_var_t* vars);

/* ---------------------------------------------------------------------------------------
 * (f2) numpy files of the TF2 exchange (host only). The TF2 consensus / parameter-server modules
 * load each neighbour's status archive and model with np.load(..., allow_pickle=True)
 * (TF2/MNIST_dataset/consensus/consensus_v3.py:82-141, consensus_v4.py:30-95,
 * parameter_server_v2.py:83-164): results/dump_train_variables{k}.npz (np.savez, stored zip of
 * numeric .npy members) and results/dump_train_model{k}.npy (np.save of a 1-D object array of
 * per-layer ndarrays, i.e. a pickle). cfa_npy_read reads one file and locates its arrays in place:
 * a numeric .npy (kind CFA_NPY_ARRAY, one array), an object .npy whose pickle holds only numpy's
 * ndarray reconstructors and numeric elements (CFA_NPY_OBJECT, one array per element; nothing in
 * the file is executed), or a stored .npz of numeric members (CFA_NPY_ARCHIVE, CRC-checked, one
 * array per member, named without ".npy"). Anything else returns CFA_E_UNSUPPORTED (fall back to
 * np.load); truncated or corrupt files return CFA_E_INVALID. The parsed file owns the memory its
 * arrays point into.
 */
#define CFA_NPY_MAX_DIM 32
enum { CFA_NPY_ARRAY = 0, CFA_NPY_OBJECT = 1, CFA_NPY_ARCHIVE = 2 };
typedef struct {
  const char* name;   /* archive member name (without ".npy"); NULL for .npy files */
  const char* descr;  /* numpy dtype string: "<f4", "<f8", "<i8", "|b1", "|u1", ... */
  int itemsize;
  int ndim;
  int64_t shape[CFA_NPY_MAX_DIM];
  int fortran_order;
  const void* data;   /* elements in C order, or Fortran order when fortran_order */
  size_t nbytes;
} cfa_npy_array_t;
typedef struct cfa_npy cfa_npy_t;
CFA_API int cfa_npy_read(const char* path, cfa_npy_t** out);
/* The same on a file image already in memory; the arrays point into `image`, which the caller
 * keeps alive until cfa_npy_free. */
CFA_API int cfa_npy_parse(const void* image, size_t nbytes, cfa_npy_t** out);
CFA_API void cfa_npy_free(cfa_npy_t* npy);
CFA_API int cfa_npy_kind(const cfa_npy_t* npy);
CFA_API int cfa_npy_num_arrays(const cfa_npy_t* npy);
CFA_API const cfa_npy_array_t* cfa_npy_arrays(const cfa_npy_t* npy);

/* (f2) The drop-in host path of one mix as a native chunk pipeline: the local model and n
 * neighbour models arrive as per-layer fp32 arrays in pageable host memory (TF2
 * consensus_v3.py:144-157 over the loaded .npy layer lists; parameter_server_v2.py:159-161) and
 * the result goes back into per-layer arrays. The bucket range is cut into chunks of
 * chunk_elems; chunk c of every model is copied into `staging` (pinned host, chunk-major, slices
 * padded to 4 elements) by `threads` host threads while the kernel of chunk c - 1 reads its
 * slices over PCIe in place; each chunk's result lands in `out_pinned` (pinned host, P elements)
 * and is copied into out_layers as soon as its kernel is done. Each chunk runs cfa_mix_seq_f32
 * when divisors is NULL, else cfa_mix_seq_div_f32, so the result equals the single-shot mix
 * bit for bit. in_layers is model-major: model m (0 = local), layer k at
 * [m * L + k]. Returns when every output layer is written.
 * On an error return no kernel of the call is still running (the stream is drained), and the
 * host copy threads have left the caller's arrays, so they may be released; the one exception is
 * a host copy that has not finished 10 minutes after the pool's 30 s limit (the message says
 * "still copying"): the arrays passed to that call must then be kept alive.
 * cfa_host_mix_staging_elems gives the staging size one call needs. */
CFA_API size_t cfa_host_mix_staging_elems(const size_t* layer_elems, int L, int n, size_t chunk_elems);
CFA_API int cfa_host_mix_f32(float* const* out_layers, const float* const* in_layers,
                             const size_t* layer_elems, int L, int n, const float* alphas,
                             const float* divisors, float* staging, size_t staging_elems,
                             float* out_pinned, size_t chunk_elems, int threads, void* stream);

/* Host-path helpers (the per-call drop-in path): hipStreamSynchronize, and a
 * stream-ordered fetch of a device uint64 counter (e.g. a compression kept_count) into host
 * memory (pinned, for an asynchronous copy) followed by resetting the counter to zero; and one
 * asynchronous copy (the pinned staging of a batch of inputs). */
CFA_API int cfa_stream_synchronize(void* stream);
/* hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, stream): the staging copy of the host path. */
CFA_API int cfa_memcpy_async(void* dst, const void* src, size_t bytes, void* stream);
CFA_API int cfa_counter_fetch(unsigned long long* counter, unsigned long long* host_dst, void* stream);
/* Completion of a short call without hipStreamSynchronize's wake-up: cfa_stream_signal enqueues
 * a one-lane kernel that stores `value` into the 32-bit word `word_dev` (the device address of a
 * pinned host word, cfa_host_device_pointer) with a system-scope release, after the stream's
 * earlier work; cfa_wait_signal spins on the host word (acquire loads) until it reads `value`.
 * After spin_us microseconds without it, cfa_wait_signal falls back to hipStreamSynchronize(stream),
 * which also reports any error of the stream's work, and then requires the value. At the C1 call
 * shape this completes 3.5 us sooner than hipStreamSynchronize (profiles/r03v_flag_sync.jsonl).
 * The caller gives each concurrent user its own word and changes `value` at every call. */
CFA_API int cfa_stream_signal(unsigned* word_dev, unsigned value, void* stream);
CFA_API int cfa_wait_signal(const unsigned* word_host, unsigned value, void* stream, long long spin_us);

/* Host lane of the routed halo (federated_amd/hostlane.py): part of a round's halo travels
 * D2H over the sender's PCIe link into shared pinned host memory and H2D over the receiver's,
 * beside the xGMI links. cfa_host_register / cfa_host_unregister pin (hipHostRegister, mapped and
 * portable) and release a caller-mapped host range, e.g. a shared-memory segment both ranks map.
 * The sender raises a chunk's sequence number with cfa_stream_signal after its D2H copy (stream
 * ordered); the receiver's HOST thread waits for it with cfa_host_wait_word and only then enqueues
 * the H2D copy, so no wait ever parks on a GPU queue (a parked wait would hold every stream sharing
 * its hardware queue). cfa_host_wait_word polls the host word (acquire loads) until it reaches
 * `value` in sequence order ((int)(word - value) >= 0): it spins ~20 us, then sleeps in 20 us
 * steps, and returns CFA_E_TIMEOUT after `timeout_us` (> 0) without it. Host only: no HIP call. */
CFA_API int cfa_host_register(void* host, size_t bytes);
CFA_API int cfa_host_unregister(void* host);
CFA_API int cfa_host_wait_word(const unsigned* word_host, unsigned value, long long timeout_us);

/* The receive side of a host lane as a pump: one native host thread per lane walks a round's
 * operations in order. Each operation: wait until the host word `wait_word` reaches `wait_value`
 * (NULL: no wait; the same poll as cfa_host_wait_word, `timeout_us` per wait); copy `bytes` from
 * `src` to `dst` (0: none); raise `signal_word` to `signal_value` (NULL: none); record `event` (a
 * hipEvent_t, NULL: none) on the lane's stream; publish `mark` (> 0) as the round's progress.
 * GPU mode (`host_mode` 0): copies are hipMemcpyAsync on `stream`, signals cfa_stream_signal on it
 * (`signal_word` a device address), so nothing waits on a GPU queue and the caller's thread does not
 * wait either until it needs a group's rows. Host mode (1): memcpy and a release store into the host
 * word (no HIP call; the CPU tests). cfa_lane_pump_submit copies the list and returns at once
 * (CFA_E_INVALID while the previous round is still in progress); cfa_lane_pump_wait blocks until
 * `mark` has been published (mark < 0: the whole round) and returns CFA_E_TIMEOUT after
 * `timeout_us` without it. A wait of the pump that times out ends the round: that error is then
 * returned by every later wait and submit (sticky). cfa_lane_pump_destroy stops the thread
 * (interrupting a wait) and frees the pump. One caller thread per pump. */
typedef struct cfa_lane_op {
  const unsigned* wait_word;
  unsigned wait_value;
  unsigned signal_value;
  unsigned* signal_word;
  void* dst;
  const void* src;
  size_t bytes;
  void* event;
  int mark;
} cfa_lane_op;
CFA_API int cfa_lane_pump_create(void** pump, void* stream, int device, int host_mode);
CFA_API int cfa_lane_pump_submit(void* pump, const cfa_lane_op* ops, int n_ops, long long timeout_us);
CFA_API int cfa_lane_pump_wait(void* pump, int mark, long long timeout_us);
CFA_API int cfa_lane_pump_destroy(void* pump);

/* ---------------------------------------------------------------------------------------
 * (a1/a2/a5/a6) Sequential CFA mix of one device with n neighbours.
 *   out[i] = fold_j( w <- w + alphas[j] * (nbrs[j][i] - w) ), w0 = local[i]
 * Replaces:
 *   TF1/consensus/cfa.py:66-76 (per-neighbour loop :119-130, alpha = eps/N)
 *   TF1/consensus/cfa_ongraphs.py:109-119 (loop :196-213, alpha = eps/(1+n))
 *   TF1/consensus/cfa_mobilenet.py:82-91, cfa_ge_2stage.py:73-83 (stage 1, :449-466)
 *   TF2 consensus_v3.py:153-155 / consensus_v2.py:153-155 / consensus_v4.py:211-213 (weights)
 *   TF2 consensus_v3.py:236-238 / consensus_v4.py:251-253 (gradients)
 *   TF2/FL_over_MQTT/learner_consensus.py:150-153 (alpha = 1/2)
 * Bytes moved: (n + 2) * P * 4.
 */
CFA_API int cfa_mix_seq_f32(float* out, const float* local, const float* const* nbrs,
                    const float* alphas, int n, size_t P, void* stream);

/* Launch configuration of the streaming mix kernels (performance only; results are identical
 * for every configuration). */
typedef struct {
  int blocks_per_cu;  /* grid = min(tiles, CUs * blocks_per_cu); 0 = one workgroup per tile */
  int vec_per_lane;   /* 16-byte vectors per lane per bucket per tile: 1, 2, 4; 0 = auto */
  int nontemporal;    /* 1 = nontemporal (streaming) loads/stores for once-touched buckets */
} cfa_launch_t;

/* cfa_mix_seq_f32 with an explicit launch configuration (NULL = library default, from sweeps on
 * placement-calibrated buckets: one workgroup per CU and 2 vectors per lane, 1 for 3-5
 * neighbours; from 512K to 1.5M elements four workgroups per CU with 1 vector per lane, from 1.5M
 * to 8M four with 4 (up to 9 neighbours; with 2 below 3M above that); an explicit configuration
 * with vec_per_lane = 0 takes round 1's auto width). */
CFA_API int cfa_mix_seq_ex_f32(float* out, const float* local, const float* const* nbrs,
                               const float* alphas, int n, size_t P, const cfa_launch_t* launch,
                               void* stream);

/* (f1) FedAvg / parameter-server fold: w <- w + (alphas[j] * (nbrs[j] - w)) / divisors[j],
 * j = 0..n-1, each step rounded like numpy's `p + u*(x - p)/C` (fp32 multiply, then IEEE fp32
 * division by the count). Replaces TF2 parameter_server_v2.py:159-161 / parameter_server.py:154,
 * :74 (metalearning), FL_over_MQTT/PS_server.py:127-134, learner_consensus.py:150-153. */
CFA_API int cfa_mix_seq_div_f32(float* out, const float* local, const float* const* nbrs,
                                const float* alphas, const float* divisors, int n, size_t P,
                                void* stream);

/* Linear-combination mix: out[i] = coeff[0]*local[i] + sum_j coeff[j+1]*nbrs[j][i].
 * The closed form of the sequential rule (c_0 = prod(1-a_j), c_{j+1} = a_j prod_{k>j}(1-a_k)),
 * and the FedAvg / parameter-server aggregation shape
 * (TF2 parameter_server_v2.py:159-161, PS_server.py:127-134). */
CFA_API int cfa_mix_f32(float* out, const float* local, const float* const* nbrs,
                const float* coeff, int n, size_t P, void* stream);

/* Sequential mix fused with the compression epilogue of cfa_ongraphs.py:225-273.
 * The epilogue applies to elements [cbegin, cend) of the bucket (the W2 tensor), with
 * `local` as the DPCM reference (n_W_l2 is the pre-mix local, :246-247). The number of
 * elements in that range NOT replaced is ADDED to *kept_count (a device uint64; zero it
 * first). Mode CFA_COMPRESS_NONE adds (cend - cbegin). */
CFA_API int cfa_mix_seq_compress_f32(float* out, const float* local, const float* const* nbrs,
                             const float* alphas, int n, size_t P, int mode, size_t cbegin,
                             size_t cend, unsigned long long* kept_count, void* stream);

/* (a3) Standalone compression epilogue, in place on y[0..P), reference `ref` (may be NULL
 * for modes 1/4). Adds the kept count to *kept_count (device uint64). */
CFA_API int cfa_compress_epilogue_f32(float* y, const float* ref, int mode, size_t P,
                              unsigned long long* kept_count, void* stream);

/* (a1/a2/a3) TF1 mix with the reference's numpy-2 numerics, fp32 buckets in and out:
 *   step 0:  w = (double)local + alphas[0] * (double)(x_0 - local)   (x_0 - local in fp32)
 *   step j:  w = w + alphas[j] * ((double)x_j - w)                     (fp64)
 *   out = (float)w after the optional compression epilogue, evaluated on the fp64 w with the
 *   fp32 `local` as DPCM reference, on elements [cbegin, cend).
 * In the reference, eps * wf is an np.float64, so the first subtraction is fp32 and the rest of
 * the chain is promoted to fp64 (TF1/consensus/cfa.py:69-76, cfa_ongraphs.py:112-119 and the
 * compression loop :225-273, cfa_mobilenet.py:82-91, cfa_ge_2stage.py:76-83). The result is
 * the reference's fp64 result rounded once to fp32, which is what the TF1 drivers feed back
 * into their fp32 graph. alphas[j] = eps * wf_j are host doubles. kept_count (device uint64)
 * may be NULL only when mode == CFA_COMPRESS_NONE (no epilogue, no count); otherwise the
 * number of elements of [cbegin, cend) NOT replaced is ADDED to it, as in
 * cfa_mix_seq_compress_f32 (mode 0: cend - cbegin). n > CFA_MAX_FANIN chains passes through an fp64 scratch bucket
 * (8 * P bytes, stream-ordered allocation), so the result still rounds once. That allocation
 * cannot be captured: under hipGraph capture with n > CFA_MAX_FANIN this entry fails
 * (CFA_E_INVALID) and cfa_mix_tf1_ex_f32 must be used. */
CFA_API int cfa_mix_tf1_f32(float* out, const float* local, const float* const* nbrs,
                            const double* alphas, int n, size_t P, int mode, size_t cbegin,
                            size_t cend, unsigned long long* kept_count, void* stream);

/* The same TF1 chain over fp32 buckets, written UNROUNDED into an fp64 `out` (P doubles): the
 * fp64 arrays the reference itself returns when its inputs are fp32 (cfa.py:66-76 under numpy 2:
 * fp32 first subtraction, fp64 after; the epilogue in fp64). Equal to cfa_mix_tf1_f64 on the
 * widened buckets with step0_f32 = 1, at half the input bytes. n >= 1; passes above
 * CFA_MAX_FANIN chain in `out` itself (no scratch, no allocation). `out` (8 * P bytes) must not
 * overlap `local` or any neighbour (CFA_E_INVALID). */
CFA_API int cfa_mix_tf1_wide_f32(double* out, const float* local, const float* const* nbrs,
                                 const double* alphas, int n, size_t P, int mode, size_t cbegin,
                                 size_t cend, unsigned long long* kept_count, void* stream);

/* cfa_mix_tf1_f32 with a caller-owned fp64 scratch bucket (device, >= P doubles, 8-byte
 * aligned; used only when n > CFA_MAX_FANIN, may be NULL otherwise): no allocation at all. */
CFA_API int cfa_mix_tf1_ex_f32(float* out, const float* local, const float* const* nbrs,
                               const double* alphas, int n, size_t P, int mode, size_t cbegin,
                               size_t cend, unsigned long long* kept_count, double* scratch,
                               void* stream);

/* (a1-a4) TF1 mix on fp64 buckets: the reference's own TF1 arithmetic, with no rounding to fp32.
 * Under numpy 2 the reference's chain is fp64 (eps * wf is an np.float64) over whatever arrays
 * the caller and the .mat files hold, and it returns fp64 arrays. The buckets here are those
 * arrays widened to fp64 (exact for fp32 values):
 *   step 0:  w = local + alphas[0] * d,  d = step0_f32 ? (double)((float)x_0 - (float)local)
 *                                                     : x_0 - local
 *   step j:  w = w + alphas[j] * (x_j - w)
 * step0_f32 = 1 when the reference's local and first-neighbour arrays are both fp32 (numpy
 * subtracts them in fp32). The optional compression epilogue (cfa_ongraphs.py:225-273) is
 * applied in fp64 on [cbegin, cend) with `local` as DPCM reference; kept_count as in
 * cfa_mix_tf1_f32. Replaces TF1/consensus/cfa.py:69-76, cfa_ongraphs.py:112-119 + 225-273,
 * cfa_mobilenet.py:82-91, cfa_ge_2stage.py:76-83 (stage 1 of CFA-GE). */
CFA_API int cfa_mix_tf1_f64(double* out, const double* local, const double* const* nbrs,
                            const double* alphas, int n, int step0_f32, size_t P, int mode,
                            size_t cbegin, size_t cend, unsigned long long* kept_count,
                            void* stream);

/* (f1) fp64 fold of the reference's server-side chains, on fp64 buckets (fp32 arrays widened
 * exactly), one fp64 rounding per operation, w0 = local:
 *   CFA_RULE_SEQUENTIAL      w <- w + alphas[j] * (x_j - w)
 *   CFA_RULE_SEQUENTIAL_DIV  w <- w + (alphas[j] * (x_j - w)) / divisors[j]
 *   CFA_RULE_ACCUMULATE      w <- w + alphas[j] * x_j
 * Replaces the aggregation loops embedded in the reference's drivers, whose operands are fp64:
 *   TF2/FL_over_MQTT/PS_server.py:130-133 (SEQUENTIAL_DIV over the decoded fp64 payloads),
 *   TF2/FL_over_MQTT/learner_consensus.py:151-152 (SEQUENTIAL_DIV, u = 1, C = 2),
 *   TF1/federated_sample_CNN_CFA_FA.py:86-89 (ACCUMULATE from zeros, a = 1/devices),
 *   :103-110 and :130-133 (SEQUENTIAL, a = eps/devices), :280-283 (client, SEQUENTIAL, a = eps2).
 * `divisors` is read only by SEQUENTIAL_DIV. out may alias local. */
CFA_API int cfa_fold_f64(double* out, const double* local, const double* const* nbrs,
                         const double* alphas, const double* divisors, int n, int rule, size_t P,
                         void* stream);

/* (a4) CFA-GE MEWMA on fp64 buckets with the reference's numpy-2 operations
 * (cfa_ge_2stage.py:331-371, :593-621), for j = 0..n-1 in order:
 *   s_j <- init ? g_j : rho*g_j + (1-rho)*s_j
 *   W   <- W - lr(i) * (use_filtered ? s_j : g_j),  lr(i) = i < lr_split ? lr1 : lr2
 * The buckets hold the reference's arrays widened to fp64; f32_mask says which of them are fp32
 * arrays there (CFA_TF1_*_F32). rho, 1-rho and lr are Python floats in the reference, so each
 * product is computed in its array's dtype, a sum/difference is fp32 only when both operands
 * are, and a state is rounded to its array's dtype on store (as numpy's slice assignment does).
 * W and s_j are updated in place; g_j is read with element stride g_stride (NULL = all 1). */
enum { CFA_TF1_STATE_F32 = 1, CFA_TF1_GRAD_F32 = 2, CFA_TF1_W_F32 = 4 };
CFA_API int cfa_mewma_tf1_f64(double* W, double* const* s, const double* const* g,
                              const int64_t* g_stride, int n, double rho, double lr1, double lr2,
                              size_t lr_split, int init, int use_filtered, int f32_mask, size_t P,
                              void* stream);

/* (a4) CFA-GE gradient-bucket update (MEWMA), for j = 0..n-1 in order:
 *   s_j <- init ? g_j : rho*g_j + (1-rho)*s_j
 *   W   <- W - lr(i) * (use_filtered ? s_j : g_j),   lr(i) = i < lr_split ? lr1 : lr2
 * Replaces TF1/consensus/cfa_ge_2stage.py:593-621 (fast; CNN use_filtered=1, 2NN 0) and
 * :329-371 (4-stage: init=1 at epoch 1, use_filtered=0). W and s_j are updated in place.
 * g_j is read with element stride g_stride (1 = contiguous). rho is a double so that rho and
 * (1 - rho) are each rounded once to fp32, as numpy does with a Python-float hyperparameter.
 * Bytes moved: (3n + 2) * P * 4. */
CFA_API int cfa_mewma_update_f32(float* W, float* const* s, const float* const* g,
                         const int64_t* g_stride, int n, double rho, float lr1, float lr2,
                         size_t lr_split, int init, int use_filtered, size_t P, void* stream);

/* (e/f4) Sliding-window population pass: nb (1..8) consecutive devices of a ring window with hl
 * neighbours below and hr above (0..4 each), mixed with the sequential rule in one launch that
 * loads each row of the window once: (nb + hl + hr) * P * 4 bytes read and nb * P * 4 written,
 * against nb * (hl + hr + 2) * P * 4 for nb separate mixes, with identical results.
 *   rows[0 .. nb+hl+hr-1]: HOST table of device pointers, consecutive devices g0-hl .. g0+nb-1+hr
 *                          (the caller resolves ring wrap-around and halo rows);
 *   device b (0 <= b < nb) mixes local rows[b+hl] with rows[b .. b+hl-1] then
 *                          rows[b+hl+1 .. b+hl+hr] (the window order of cfa.py:14-32 /
 *                          consensus_v4.py:133-137), coefficient alphas[b] at every step (the
 *                          reference's eps policies give a window device one value:
 *                          1/(K+1), consensus_v3.py:145; eps*b/(b + m*b), cfa.py:66-68);
 *   out[0 .. nb-1]: HOST table of output device pointers (must not alias any row). */
CFA_API int cfa_mix_window_f32(float* const* out, const float* const* rows, const float* alphas,
                               int nb, int hl, int hr, size_t P, void* stream);

/* (e/f4) A whole ring-window round of a STACKED population in one launch: device d's model is
 * in + d * pitch (P floats), its output out + d * pitch; every device mixes with the ring window
 * [d-hl .. d-1, d+1 .. d+hr] (mod D) in that order with coefficient alphas[d] (DEVICE array of D
 * floats) at each step. The devices run as cfa_mix_window_f32 passes of 8 consecutive devices,
 * all passes in the same launch; results are identical to those passes and to D per-device
 * sequential mixes. Rows must be 16-byte aligned (pitch and P multiples of 4); out must not
 * overlap in. */
CFA_API int cfa_mix_ring_round_f32(float* out, const float* in, size_t pitch, const float* alphas, int D,
                                   int hl, int hr, size_t P, void* stream);

/* (e/f4) A run of consecutive ring devices of a STACKED population with every row read once and
 * every output written once: devices first .. first+count-1 of a stack of `rows` rows (row r of the
 * input at in + r * in_pitch, of the output at out + r * out_pitch, P floats each). Device d mixes
 * its row with rows (d-hl .. d-1, d+1 .. d+hr) mod rows in that order, coefficient
 * alphas[d - first] (DEVICE array of count floats) at each step, and writes row d mod rows of out;
 * the run may pass the last row only when count == rows (the whole ring). Each workgroup slides a
 * register window of hl+hr+1 rows down a segment of the run, so a call moves
 * (2 * count + segments * (hl+hr)) * P * 4 bytes against count * (hl+hr+2) * P * 4 for per-device
 * mixes, with identical results. Launch shape (environment, read at each launch, results
 * identical): CFA_SLIDE_SEGMENTS, CFA_SLIDE_WG_PER_CU, CFA_SLIDE_PF (rows prefetched, 1..4),
 * CFA_SLIDE_SC1 (write-through stores). CFA_E_UNSUPPORTED unless rows are 16-byte aligned (bases,
 * pitches and P multiples of 4 floats); out must not overlap in. */
CFA_API int cfa_mix_ring_slide_f32(float* out, size_t out_pitch, const float* in, size_t in_pitch,
                                   const float* alphas, int rows, int first, int count, int hl, int hr,
                                   size_t P, void* stream);

/* (f3) CFA-GE neighbour-gradient evaluation: the gradient of a device's own cost at each of M
 * neighbour models, for the two TF1 graphs of cfa_ge_2stage.py (:391-433 graph, :512-528 one
 * Session per neighbour; cfa_ge_4stage.py the same), one workgroup per model, fp32 like the
 * reference's placeholders. x [B, L] and y [B, classes] are the device's samples and one-hot
 * labels (x_train2, y_train2); models [M, P] and grads [M, P] are model buckets in the TF1
 * order (W1, b1, W2, b2), all device arrays.
 *   CNN (ML_model 1): W1 [filter, 1, number], conv stride = pool size = `stride`, SAME padding,
 *       W2 [L2 * number, classes] with L2 = ceil(ceil(L / stride) / stride) (the reference's
 *       `multip`); P = filter*number + number + L2*number*classes + classes.
 *   2NN (ML_model 2): W1 [L, hidden], W2 [hidden, classes]; P = L*hidden + hidden + hidden*classes + classes.
 * cost = mean_b(-sum_c y log(clip(softmax, 1e-15, 0.99))) (:425-426). CFA_E_UNSUPPORTED when the
 * activations of B samples do not fit one workgroup's LDS. */
CFA_API int cfa_ge_grad_cnn_f32(const float* x, const float* y, int B, int L, int classes, int filter,
                                int number, int stride, const float* models, float* grads, int M,
                                void* stream);
CFA_API int cfa_ge_grad_2nn_f32(const float* x, const float* y, int B, int L, int hidden, int classes,
                                const float* models, float* grads, int M, void* stream);
/* Population form: evaluation m uses model row model_row[m] of models [Dm, P] and data row
 * data_row[m] of x [Dx, B, L] / y [Dx, B, classes] (DEVICE int32 tables), writing grads[m]. One
 * launch evaluates every (device, neighbour) pair of a device-resident CFA-GE population: the
 * gradient of device data_row[m]'s cost at device model_row[m]'s published model. With a device
 * `workspace` of at least cfa_ge_grad_workspace_elems(M, B, P) floats, each evaluation's batch is
 * split over several workgroups (about two per CU in all) whose partial sums are then added in a
 * fixed order (deterministic); with less (or NULL) one workgroup takes each evaluation.
 * grads == NULL: partials only. The launch writes [M][S][P] partial buckets to `workspace`
 * (S = cfa_ge_grad_splits(M, B, P); at least M * S * P floats) and the caller sums them, e.g. in
 * the same launch as the next population step (cfa_ge_population_step_f32's reduce_* args). */
CFA_API int cfa_ge_grad_splits(int M, int B, size_t P);
CFA_API size_t cfa_ge_grad_workspace_elems(int M, int B, size_t P);
CFA_API int cfa_ge_grad_cnn_rows_f32(const float* x, const float* y, int B, int L, int classes,
                                     int filter, int number, int stride, const float* models,
                                     const int32_t* model_row, const int32_t* data_row, float* grads,
                                     float* workspace, size_t workspace_elems, int M, void* stream);
CFA_API int cfa_ge_grad_2nn_rows_f32(const float* x, const float* y, int B, int L, int hidden,
                                     int classes, const float* models, const int32_t* model_row,
                                     const int32_t* data_row, float* grads, float* workspace,
                                     size_t workspace_elems, int M, void* stream);

/* (f3/f4) Local training between two rounds: one epoch of plain minibatch SGD for every device
 * of a TF1 population in one launch (federated_sample_CNN_CFA-GE.py:137-173, the assignment
 * W <- W_ext - learning_rate * grad :114-118; federated_sample_2NN_CFA.py:97-101), on the two
 * graphs and the cost of the cfa_ge_grad_* block above. x [D, Ns, L] and y [D, Ns, classes] are
 * every device's samples and one-hot labels; models is a [D, pitch] stack of model buckets in
 * the TF1 order (W1, b1, W2, b2), pitch >= P floats, all device fp32 arrays. One workgroup owns
 * device d for the whole launch and keeps its model in LDS:
 *   w = models[d]
 *   for i in 0 .. steps-1: minibatch i = sample rows [i*batch_stride, i*batch_stride + batch_rows)
 *       c_i = cost(w; minibatch i), a mean over batch_rows
 *       update != 0:  w <- w - lr * d cost / d w      (fp32)
 *   update != 0:  models[d] = w      (update == 0: the validation pass :163-172, forward only,
 *                                     models untouched)
 *   cost[d] = sum_i c_i / steps      (fp64, like the driver's Python float; cost may be NULL)
 * The driver's slice i*batch_size : (i+1)*batch_size - 1 is batch_stride 5, batch_rows 4.
 * cost_log [log_cap, D] (fp64) and epoch (one device counter) are given together or both NULL:
 * with them the launch also writes cost[d] to row min(*epoch, log_cap-1) of cost_log and leaves
 * *epoch one higher in stream order, so a replayed graph of many epochs leaves the whole curve
 * on the device. Deterministic: every output has one owner, every sum a fixed order.
 * CFA_E_INVALID: steps, batch_rows or batch_stride < 1, a minibatch past Ns, pitch < P, a null
 * x / y / models. CFA_E_UNSUPPORTED: the model, two minibatches and their activations exceed
 * one workgroup's LDS (raised to the device's 160 KiB by cfa_device_prepare), or classes > 64. */
CFA_API int cfa_local_sgd_cnn_f32(const float* x, const float* y, int Ns, int L, int classes, int filter,
                                  int number, int stride, float* models, size_t pitch, int D,
                                  int batch_stride, int batch_rows, int steps, float lr, int update,
                                  double* cost, double* cost_log, int log_cap, unsigned long long* epoch,
                                  void* stream);
CFA_API int cfa_local_sgd_2nn_f32(const float* x, const float* y, int Ns, int L, int hidden, int classes,
                                  float* models, size_t pitch, int D, int batch_stride, int batch_rows,
                                  int steps, float lr, int update, double* cost, double* cost_log,
                                  int log_cap, unsigned long long* epoch, void* stream);

/* (TF2 drivers) The local optimizer step between two rounds, for every device of a TF2
 * population in one call: what optimizer.apply_gradients(zip(grads, model.trainable_variables))
 * does on each device (federated_learning_keras_consensus_FL_MNIST.py:363-381) with the three
 * optimizers the drivers construct. The gradients are the caller's.
 *   models [D, pitch] fp32, stepped in place; grads [D, grad_pitch] fp32, read only; m, v
 *           [D, state_pitch] fp32, the caller's state (SGD: neither is read and both may be NULL;
 *           momentum: m is the accumulator, v may be NULL). All DEVICE arrays with unit element
 *           stride and pitches >= P. A device whose rows all start 16-byte aligned is streamed in
 *           16-byte vectors, any other element by element, with the same results.
 *   layer_ptr [n_layers + 1] int32 (DEVICE), 0 = layer_ptr[0] < ... < layer_ptr[n_layers] = P:
 *           the layers of a row in get_weights() order, boundaries arbitrary. Device memory: not
 *           checked here, the caller checks the table before the upload (whatever it holds, no
 *           access leaves a row or the workspace).
 *   trainable [n_layers] int32 (DEVICE): a layer with 0 is neither read nor written.
 *   skip    [D] int32 (DEVICE) or NULL: a device with a non-zero flag is not touched at all, its
 *           model, state, t and pow stay as they are (the populations' training_end flags).
 *   t       [D] int64 (DEVICE): steps taken by each device, left one higher for every device
 *           stepped, in stream order.
 *   pow     [D, 2] fp64 (DEVICE; Adam only): beta_1^t and beta_2^t, 1 at t = 0, multiplied up
 *           once per step by the call.
 * rule (every fp32 operation rounded on its own, no contraction):
 *   CFA_OPTIM_SGD:      w <- w - lr * g
 *   CFA_OPTIM_MOMENTUM: a <- momentum * a - lr * g; w <- w + a        (a is m; not Nesterov)
 *   CFA_OPTIM_ADAM:     per device and trainable layer, when clipnorm > 0, s = sum g^2 (fp64, a
 *       fixed order, no atomics), g' = g * RN_32(clipnorm / max(sqrt(s), clipnorm)) as
 *       tf.clip_by_norm does (the factor is exactly 1 at or below the norm; an all-zero layer
 *       stays zero); clipnorm <= 0: g' = g and no norm pass. Then, with t counted from 1,
 *       lr_t = RN_32(lr * sqrt(1 - beta_2^t) / (1 - beta_1^t)) formed in fp64,
 *       m <- m + (g' - m) * RN_32(1 - beta_1); v <- v + (g' * g' - v) * RN_32(1 - beta_2);
 *       w <- w - lr_t * m / (sqrt(v) + epsilon), all fp32.
 * workspace: the clip's partial sums, at least cfa_optim_workspace_bytes(D, P, n_layers) bytes of
 * DEVICE memory (NULL without the clip): one fp64 partial per tile of cfa_optim_tile() elements
 * and layer it meets; tiles are counted from a row's first element. The same inputs give the
 * same bits on every run. No host read, allocation or attribute call: capture-safe. Two launches
 * and the counters' (three with the clip), none per layer or per device.
 * CFA_E_INVALID: an unknown rule, D, P or n_layers < 1, a null array the rule needs, a pitch
 * below P, beta_1 or beta_2 outside [0, 1), a non-finite lr or momentum, a negative epsilon, a
 * workspace too small for the clip. CFA_E_UNSUPPORTED: an array that is not aligned to its
 * element size, P beyond the int32 table, D > 65535. */
CFA_API int cfa_optim_tile(void);
CFA_API size_t cfa_optim_workspace_bytes(int D, size_t P, int n_layers);
CFA_API int cfa_optim_step_f32(float* models, size_t pitch, const float* grads, size_t grad_pitch, float* m,
                               float* v, size_t state_pitch, const int32_t* layer_ptr,
                               const int32_t* trainable, int n_layers, const int32_t* skip, long long* t,
                               double* pow, int rule, float lr, float momentum, double beta_1, double beta_2,
                               float epsilon, float clipnorm, void* workspace, size_t workspace_bytes, int D,
                               size_t P, void* stream);

/* (TF2 drivers) The validation pass of a LeNet-1 population and the training_end flag it raises:
 * what every device does once per epoch in
 * federated_learning_keras_consensus_FL_threads_MNIST_crossentropy_gradients_exchange.py:430-455
 * with the model of create_q_model, condition 0 (:158-194). Forward only: the gradient is cfa_lenet_grad_f32.
 * The model family, Keras semantics, geometry (side, kernel, c1, c2, classes):
 *   x [side, side, 1] -> Conv2D(c1, kernel x kernel, valid, relu) -> AveragePooling2D(2 x 2)
 *     -> Conv2D(c2, kernel x kernel, valid, relu) -> AveragePooling2D(2 x 2) -> Flatten (NHWC)
 *     -> Dense(classes, softmax)
 * Conv2D is a cross-correlation with the kernel tensor (kh, kw, in, out); pooling drops an odd
 * last row and column. A model row is get_weights() order, C-order: K1 (k,k,1,c1), b1, K2
 * (k,k,c1,c2), b2, Wd (flat, classes), bd, with s1 = side-k+1, p1 = s1/2, s2 = p1-k+1, p2 = s2/2,
 * flat = p2*p2*c2 and P = k*k*c1 + c1 + k*k*c1*c2 + c2 + flat*classes + classes = cfa_lenet_params
 * (0 for a geometry without a model). LeNet-1 is (28, 5, 4, 8, 10), P = 2202.
 *   x       [Nt, side, side] fp32 and labels [Nt] int32 (values in [0, classes); the caller
 *           checks them: a label outside gives a NaN cost): the test set all devices share, with
 *           both device strides 0. A non-zero stride (in elements) gives device d its own set at
 *           x + d * x_dev_stride / labels + d * label_dev_stride.
 *   models  [D, pitch] fp32, pitch >= P, read only; rows need no alignment.
 *   skip    [D] int32 or NULL: a device with a non-zero flag has left its loop (:498); its cost
 *           and flag are not touched.
 * For every other device d:
 *   for b in 0 .. batches-1: loss_b = mean over samples [b*batch, (b+1)*batch) of
 *       -log softmax(z)[label]                                    (fp32)
 *   cost[d] = (sum_b (double)loss_b) / batches                    (fp64, in batch order)
 *   ended != NULL: ended[d] = ended[d] | (cost[d] < target)
 * skip and ended may be the same array (a population's flags): each flag has one owner, which
 * reads it before writing it. cost_log [log_cap, D] (fp64) and epoch (one device counter) are
 * given together or both NULL and work as in the cfa_local_sgd_* block: row min(*epoch, log_cap-1)
 * receives every device's cost[d] (a skipped device's untouched one) and *epoch is left one higher
 * in stream order. workspace: at least cfa_lenet_eval_workspace_bytes(D, batches) bytes of DEVICE
 * memory (the fp32 batch losses).
 * Every operation is fp32 (no contraction); the log-probability is z - max - log(sum exp(z - max)).
 * The reference takes log of the softmax output (:442): the two agree to rounding wherever no
 * class probability underflows; where one does the reference yields inf / nan and this a finite
 * cost. Its avg_cost += loss / n is fp32 under numpy 2 and fp64 under numpy 1: fp64 here.
 * Deterministic: every output has one owner and every sum a fixed order, no atomics; a batch's
 * loss depends neither on how batches are dealt to workgroups nor on d. No host read, allocation
 * or attribute call: capture-safe. Two launches, none per device, batch or layer.
 * CFA_E_INVALID: a null x, labels, models, cost or workspace; D, batch, batches, c1, c2, classes
 * or kernel < 1; a geometry with p2 < 1; batch*batches > Nt; pitch < P; a non-zero device stride
 * below one device's set; only one of cost_log / epoch; a workspace too small; a non-finite target
 * with ended. CFA_E_UNSUPPORTED: classes > 64, D > 65535, or a model, four samples' activations
 * and a batch of losses beyond one workgroup's LDS (raised to the device's 160 KiB by
 * cfa_device_prepare), e.g. (28, 3, 32, 64, 10) with P = 34826: refused, not approximated. */
CFA_API size_t cfa_lenet_params(int side, int kernel, int c1, int c2, int classes);  /* 0: invalid geometry */
CFA_API size_t cfa_lenet_eval_workspace_bytes(int D, int batches);
CFA_API int cfa_lenet_eval_f32(const float* x, size_t x_dev_stride, const int32_t* labels, size_t label_dev_stride,
                               int Nt, int side, int kernel, int c1, int c2, int classes,
                               const float* models, size_t pitch, int D, int batch, int batches,
                               const int32_t* skip, double target, int32_t* ended,
                               double* cost, double* cost_log, int log_cap, unsigned long long* epoch,
                               void* workspace, size_t workspace_bytes, void* stream);

/* The same pass on the objective `loss` (CFA_LENET_LOSS_*); cfa_lenet_eval_f32 is this call with
 * CFA_LENET_LOSS_XENT, bit for bit. CFA_LENET_LOSS_HUBER is the objective of the drivers that
 * train LeNet-1 with keras.losses.Huber() (federated_learning_keras_consensus_FL_MNIST.py:125,
 * validation :481-483; ..._FL_threads_MNIST_gradients_exchange.py:442-447; the PS drivers): the
 * Huber loss, delta = 1, between the integer label ITSELF, cast to float, and the softmax
 * probability of the true class. Per sample with label l:
 *   p = exp(z_l - max) / sum_c exp(z_c - max);  e = p - (float)l          (fp32, classes in order)
 *   h = 0.5 e^2 where |e| <= 1, else |e| - 0.5
 * and loss_b is the mean of h over the batch, summed and divided as above. With 0 < p < 1 the
 * label picks the branch (0: quadratic in p; 1: quadratic in 1 - p; 2 and above: linear). Where p
 * rounds to exactly 0 or 1, e reaches a branch's edge; <= keeps the quadratic branch, as Keras
 * does, and both branches have the same value and slope there. A label outside [0, classes) gives
 * a NaN cost. Every other argument, the workspace, the determinism and the refusals are those of
 * cfa_lenet_eval_f32; CFA_E_INVALID also for an unknown loss (checked first, before any buffer). */
CFA_API int cfa_lenet_eval_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                    size_t label_dev_stride, int Nt, int side, int kernel, int c1, int c2,
                                    int classes, const float* models, size_t pitch, int D, int batch, int batches,
                                    const int32_t* skip, double target, int32_t* ended,
                                    double* cost, double* cost_log, int log_cap, unsigned long long* epoch,
                                    void* workspace, size_t workspace_bytes, int loss, void* stream);

/* (TF2 drivers) A minibatch's loss and gradient for every device of a LeNet-1 population, the
 * model family, row layout and geometry of the block above: the local update's
 *   loss = reduce_mean(-sum(onehot * log(model(x)))); grads = tape.gradient(loss, weights)
 * (..._MNIST_crossentropy_gradients_exchange.py:321-337), and the gradient a device evaluates at a
 * neighbour's model on a batch of its own data (:360-385). The optimizer step is cfa_optim_step_f32.
 *   x, labels, Nt, strides: the training set, shared (strides 0) or one per device, as above.
 *   models  [D, pitch] fp32, pitch >= P, read only.
 *   src     [D] int32 DEVICE array or NULL: device d evaluates row src[d] of models on its OWN
 *           data (:360-385); NULL: row d. A value outside [0, D) is the caller's error (nothing is
 *           read through it; that device's row and loss become NaN).
 *   first   [D] int64 DEVICE array or NULL: the index of the first sample of device d's batch
 *           (NULL: 0), on the device so that a captured epoch can advance it. Sample s of the batch
 *           is sample (first[d] + s) mod Nt of the set: a batch past the set's end wraps.
 *   skip    [D] int32 or NULL: a flagged device does no work; its grads row and loss are untouched.
 *   grads   [D, gpitch] fp32, gpitch >= P, any alignment; elements P.. of a row are not written.
 *   loss    [D] fp32 or NULL: the batch's mean loss.
 * For every other device, per sample with label l and logits z (fp32, explicit fma, fixed order):
 *   dz[c] = exp(z_c - max) / sum - (c == l); dWd = flat (x) dz; dbd = dz; dflat = Wd dz;
 *   average pool backward: 0.25 d(pooled) to each window position, 0 to a dropped row or column;
 *   relu gate z > 0 (the forward's own test); dK[ky][kx][ci][co] = sum_{y,x} in[y+ky][x+kx][ci] dzc[y][x][co];
 *   db[co] = sum_{y,x} dzc[y][x][co]; stage 2's input gradient the transposed correlation.
 *   grads[d] = (sum over the batch) / batch, loss[d] = (sum of the samples' losses, in order) / batch,
 * the loss bit for bit the batch loss of cfa_lenet_eval_f32 on the same samples.
 * Deterministic, no atomics: the batch is cut into groups of 4 samples whatever D, skip, src or the
 * GPU are, a group's sums have a fixed order and the groups are added in order, so a device's row
 * has the same bits alone or in a population. A label outside [0, classes) reads nothing out of
 * bounds and makes that device's loss and whole row NaN. workspace: at least
 * cfa_lenet_grad_workspace_bytes(D, batch, geometry) bytes of DEVICE memory (0 for D or batch < 1
 * or a geometry without a model). No host read, allocation or attribute call after
 * cfa_device_prepare: capture-safe. Two launches.
 * CFA_E_INVALID: a null x, labels, models, grads or workspace; D, batch or Nt < 1; a bad geometry;
 * batch > Nt; pitch or gpitch < P; a non-zero device stride below one device's set; a workspace
 * too small. CFA_E_UNSUPPORTED: classes > 64, D > 65535, or a model, its gradient and two
 * samples' activations beyond one workgroup's LDS, e.g. (28, 3, 32, 64, 10): refused. */
CFA_API size_t cfa_lenet_grad_workspace_bytes(int D, int batch, int side, int kernel, int c1, int c2, int classes);
CFA_API int cfa_lenet_grad_f32(const float* x, size_t x_dev_stride, const int32_t* labels, size_t label_dev_stride,
                               int Nt, int side, int kernel, int c1, int c2, int classes,
                               const float* models, size_t pitch, int D, const int32_t* src,
                               const long long* first, int batch, const int32_t* skip,
                               float* grads, size_t gpitch, float* loss,
                               void* workspace, size_t workspace_bytes, void* stream);

/* The same gradient on the objective `loss_kind` (CFA_LENET_LOSS_*); cfa_lenet_grad_f32 is this
 * call with CFA_LENET_LOSS_XENT, bit for bit. CFA_LENET_LOSS_HUBER: the local update of the Huber
 * drivers,
 *   class_v = reduce_sum(classes * masks, axis=1); loss = Huber()(label_sample, class_v)
 * (federated_learning_keras_consensus_FL_MNIST.py:369-377;
 * ..._FL_threads_MNIST_gradients_exchange.py:327-335, and at a neighbour's model :364-380), with
 * p, e and h of cfa_lenet_eval_loss_f32 and, at the logits,
 *   dz[c] = (g p) ((c == l) - exp(z_c - max) / sum),  g = e where |e| <= 1, else sign(e);
 * everything behind dz, the 1 / batch factor, the groups of 4 samples and the loss's bit-for-bit
 * agreement with cfa_lenet_eval_loss_f32 on the same samples are as above. A label outside
 * [0, classes) makes that device's loss and whole row NaN. CFA_E_INVALID also for an unknown
 * loss_kind (checked first, before any buffer). */
CFA_API int cfa_lenet_grad_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                    size_t label_dev_stride, int Nt, int side, int kernel, int c1, int c2,
                                    int classes, const float* models, size_t pitch, int D, const int32_t* src,
                                    const long long* first, int batch, const int32_t* skip,
                                    float* grads, size_t gpitch, float* loss,
                                    void* workspace, size_t workspace_bytes, int loss_kind, void* stream);

/* (TF2 drivers) The same two passes for create_q_model's MAX-POOL CNNs, conditions 1 and 2 of
 * -modelselection (..._MNIST_crossentropy_gradients_exchange.py:170-182 for the model; :321-337 the
 * local update, :360-385 the gradient at a neighbour's model, :430-455 the validation pass):
 *   x [side, side, 1] -> Conv2D(c1, kernel x kernel, valid, relu) -> MaxPooling2D(2 x 2, stride 2, valid)
 *     -> Conv2D(c2, kernel x kernel, valid, relu) -> MaxPooling2D(2 x 2) -> Flatten (NHWC)
 *     -> Dense(classes, softmax)
 * with (28, 3, 32, 64, 10), P = 34826, for condition 1 and (28, 3, 14, 64, 10), P = 24278, for any
 * other value (28 -> 26 -> 13 -> 11 -> 5, flat = 1600: the second pool drops a row and a column).
 * Geometry, row layout, P (cfa_lenet_params), the cross-correlation, the bias added last, the
 * z > 0 relu gate, both objectives, the log-softmax form, NaN for a label outside [0, classes)
 * and every argument are those of cfa_lenet_eval_loss_f32 / cfa_lenet_grad_loss_f32; the argument
 * lists are theirs. What differs:
 *   forward:  pooled = max over the window of relu(z); an odd last row and column are dropped.
 *   backward: the whole of d(pooled) goes to ONE position of the window, the FIRST maximum of
 *             relu(z) in window order (0,0), (0,1), (1,0), (1,1) (TF's MaxPoolGrad), and then
 *             through that position's relu gate: a window whose maximum is 0 passes nothing,
 *             wherever its tie falls. A dropped row or column receives 0. The decision is kept as
 *             one byte per pooled element (position and gate bit) and applied as a product with
 *             1 or 0, so a NaN upstream (a label out of range) reaches the device's whole row.
 * The model is NOT held in LDS: weights are read from global memory (a [D, P] stack stays in L2 /
 * the Infinity Cache); LDS holds a chunk's activations, their gradients and the decisions, the
 * chunk sized from the geometry and the device's LDS. Every operation is fp32 (explicit fma, no
 * contraction, no matrix instructions).
 * Deterministic, no atomics: every sum has a fixed order that depends on the geometry and the
 * batch alone (a sample's sums are its own; the gradient kernel adds samples in order within
 * groups of 8 and the groups in order), so a device's cost, loss and gradient row have the same
 * bits alone or in a population, whatever D, skip, src, first or the GPU's CU count and LDS
 * are, and the loss of the gradient call is bit for bit the batch loss of the validation call on
 * the same samples. No host read, allocation or attribute call after cfa_device_prepare:
 * capture-safe. Two launches per call.
 * workspace: at least cfa_lenet_max_eval_workspace_bytes(D, batches) (the fp32 batch losses) or
 * cfa_lenet_max_grad_workspace_bytes(D, batch, geometry) bytes of DEVICE memory (the groups'
 * gradient sums: D * ceil(batch / 8) * (P + 8) floats; 0 for D, batch(es) < 1 or a geometry
 * without a model).
 * Errors, in the siblings' order: CFA_E_INVALID for an unknown loss (checked first, before any
 * buffer), then for a null buffer, D, batch, batches or Nt < 1, a bad geometry, batch*batches > Nt
 * (batch > Nt), pitch or gpitch < P, a short device stride, only one of cost_log / epoch, a
 * workspace too small, a non-finite target with ended; CFA_E_UNSUPPORTED for classes > 64,
 * D > 65535, and only then for ONE sample's state beyond a workgroup's LDS (validation: image,
 * two pooled maps, logits and the batch's losses; gradient: those, their gradients and the gated
 * map of stage 2). The average-pool entries above keep refusing these geometries. */
CFA_API size_t cfa_lenet_max_eval_workspace_bytes(int D, int batches);
CFA_API int cfa_lenet_max_eval_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                        size_t label_dev_stride, int Nt, int side, int kernel, int c1, int c2,
                                        int classes, const float* models, size_t pitch, int D, int batch, int batches,
                                        const int32_t* skip, double target, int32_t* ended,
                                        double* cost, double* cost_log, int log_cap, unsigned long long* epoch,
                                        void* workspace, size_t workspace_bytes, int loss, void* stream);
CFA_API size_t cfa_lenet_max_grad_workspace_bytes(int D, int batch, int side, int kernel, int c1, int c2, int classes);
CFA_API int cfa_lenet_max_grad_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                        size_t label_dev_stride, int Nt, int side, int kernel, int c1, int c2,
                                        int classes, const float* models, size_t pitch, int D, const int32_t* src,
                                        const long long* first, int batch, const int32_t* skip,
                                        float* grads, size_t gpitch, float* loss,
                                        void* workspace, size_t workspace_bytes, int loss_kind, void* stream);

/* (TF2 drivers) The same two passes for the CIFAR drivers' HIDDEN-LAYER LeNet, -modelselection 1 of
 * federated_learning_keras_consensus_FL_threads_CIFAR_crossentropy.py:179-186 and of
 * ..._CIFAR_crossentropy_gradients_exchange.py (elif condition == 1), a family of SEVEN numbers
 * (side, channels, kernel, c1, c2, hidden, classes):
 *   x [side, side, channels] -> Conv2D(c1, kernel x kernel, valid, relu) -> AveragePooling2D(2 x 2)
 *     -> Conv2D(c2, kernel x kernel, valid, relu) -> AveragePooling2D(2 x 2) -> Flatten (NHWC)
 *     -> Dense(hidden, relu) -> Dense(classes, softmax)
 * with (32, 3, 5, 4, 8, 128, 10) for the drivers: 32 -> 28 -> 14 -> 10 -> 5, flat = 200 and
 * P = 304 + 808 + 25728 + 1290 = 28130 (cfa_lenet_hidden_params; 0 for a geometry without a model:
 * a dimension below 1, hidden included, or a second pooled map below 1 x 1).
 *   x       [Nt, side, side, channels] fp32, NHWC, shared (x_dev_stride 0), or one set per device
 *           x_dev_stride >= Nt * side * side * channels floats apart.
 *   models  [D, pitch]: a row is get_weights() order, C-order, eight tensors:
 *           K1 (k, k, channels, c1), b1, K2 (k, k, c1, c2), b2, Wh (flat, hidden), bh,
 *           Wd (hidden, classes), bd, with flat = p2 * p2 * c2 and Flatten index (y * p2 + x) * c2 + c.
 * The convolutions, the average pool (an odd last row and column dropped; backward 0.25 d(pooled)
 * to each kept position), the z > 0 relu gates, both objectives, the log-softmax form, NaN for a
 * label outside [0, classes) and every other argument are those of cfa_lenet_eval_loss_f32 /
 * cfa_lenet_grad_loss_f32. What is new:
 *   forward:  h[j] = relu(sum_i flat[i] Wh[i][j] + bh[j]); z = h Wd + bd.
 *   backward: dh[j] = (sum_c Wd[j][c] dz[c]) where the forward's own h[j] > 0 (TF's ReluGrad; the
 *             gate is not stored, h > 0 exactly where its pre-activation was; applied as a product
 *             with 1 or 0, so a NaN upstream reaches the whole row), dWh = flat (x) dh, dbh = dh,
 *             dflat[i] = sum_j Wh[i][j] dh[j].
 * The model is NOT held in LDS (the plan of the max-pool entries): weights are read from global
 * memory with the output index innermost, LDS holds a chunk's activations, their gradients, the
 * pools' gate bytes and the hidden layer's partial sums. fp32, explicit fma, no matrix instructions.
 * Deterministic, no atomics: every sum has a fixed order that depends on the geometry alone (a
 * hidden sum is cut into at most 16 interleaved slices from hidden and the workgroup size, added
 * in order; the gradient kernel adds samples in order within groups of 8 and the groups in
 * order), so a device's cost, loss and gradient row have the same bits alone or in a population,
 * whatever D, skip, src, first or the GPU's CU count and LDS are, and the loss of the gradient
 * call is bit for bit the batch loss of the validation call on the same samples. No host read,
 * allocation or attribute call after cfa_device_prepare: capture-safe. Two launches per call.
 * Accuracy is that of fp32 sums in this order: about 1e-6 normwise per tensor of the fp64 value on
 * well-conditioned tensors; a bias gradient whose terms of both signs cancel to a thousandth of
 * their size keeps about 5e-5 (measured), as any fp32 sum of them would.
 * workspace: at least cfa_lenet_hidden_eval_workspace_bytes(D, batches) or
 * cfa_lenet_hidden_grad_workspace_bytes(D, batch, geometry) bytes of DEVICE memory
 * (D * ceil(batch / 8) * (P + 8) floats; 0 for D, batch(es) < 1 or a geometry without a model).
 * Errors, in the siblings' order: CFA_E_INVALID for an unknown loss (checked first, before any
 * buffer), then for a null buffer, D, batch, batches or Nt < 1, a bad geometry, batch*batches > Nt
 * (batch > Nt), pitch or gpitch < P, a short device stride, only one of cost_log / epoch, a
 * workspace too small, a non-finite target with ended; CFA_E_UNSUPPORTED for classes > 64,
 * D > 65535, and only then for ONE sample's state beyond a workgroup's LDS (validation: image,
 * two pooled maps, h, logits, the partial sums and the batch's losses; gradient: those, their
 * gradients and the gated map of stage 2; the gradient entry checks its workspace after this). */
CFA_API size_t cfa_lenet_hidden_params(int side, int channels, int kernel, int c1, int c2, int hidden, int classes);
CFA_API size_t cfa_lenet_hidden_eval_workspace_bytes(int D, int batches);
CFA_API int cfa_lenet_hidden_eval_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                           size_t label_dev_stride, int Nt, int side, int channels, int kernel,
                                           int c1, int c2, int hidden, int classes, const float* models,
                                           size_t pitch, int D, int batch, int batches, const int32_t* skip,
                                           double target, int32_t* ended, double* cost, double* cost_log,
                                           int log_cap, unsigned long long* epoch, void* workspace,
                                           size_t workspace_bytes, int loss, void* stream);
CFA_API size_t cfa_lenet_hidden_grad_workspace_bytes(int D, int batch, int side, int channels, int kernel, int c1,
                                                     int c2, int hidden, int classes);
CFA_API int cfa_lenet_hidden_grad_loss_f32(const float* x, size_t x_dev_stride, const int32_t* labels,
                                           size_t label_dev_stride, int Nt, int side, int channels, int kernel,
                                           int c1, int c2, int hidden, int classes, const float* models,
                                           size_t pitch, int D, const int32_t* src, const long long* first,
                                           int batch, const int32_t* skip, float* grads, size_t gpitch,
                                           float* loss, void* workspace, size_t workspace_bytes, int loss_kind,
                                           void* stream);

/* (a1-a6 batched) Population round: one launch mixes D devices.
 * For device d, CSR entries e in [csr_ptr[d], csr_ptr[d+1]) list its sources in order; the
 * FIRST entry is the device's own (local) bucket. Source e is src_ptrs[csr_idx[e]], output d
 * is out_ptrs[d]; both tables are DEVICE arrays of device pointers. rule:
 *   CFA_RULE_SEQUENTIAL: w = src(first); w <- w + csr_coef[e]*(src(e) - w) for later e
 *   CFA_RULE_LINEAR:     out = sum_e csr_coef[e] * src(e)
 * csr_ptr/csr_idx/csr_coef are DEVICE arrays. Outputs must not alias any source. */
CFA_API int cfa_mix_population_f32(float* const* out_ptrs, const float* const* src_ptrs,
                           const int32_t* csr_ptr, const int32_t* csr_idx,
                           const float* csr_coef, int D, int rule, size_t P, void* stream);

/* (a1/a2 batched) TF1 population round: as cfa_mix_population_f32 with the TF1 modules'
 * numerics (cfa.py:66-76 under numpy 2): per device d, w = local; the first neighbour step
 * subtracts in fp32, every later operation is fp64 with csr_coef[e] (DEVICE double array, the
 * np.float64 products eps * wf_j; entry e0's coefficient unused), and the result is rounded to
 * fp32 once: what a TF1 driver's fp32 variables hold after assigning the reference's arrays.
 * mode != CFA_COMPRESS_NONE: the cfa_ongraphs compression epilogue (cfa_ongraphs.py:225-273)
 * on elements [cbegin, cend) of every device (the W2 segment), against the device's pre-mix
 * local, before the rounding, as cfa_mix_tf1_f32 applies it; a device without neighbours gets
 * the fp32 epilogue on its local. kept_counts[d] (DEVICE, D counters, zeroed by the caller)
 * += device d's counter_param. Buckets 16-byte aligned; outputs must not alias any source. */
CFA_API int cfa_mix_population_tf1_f32(float* const* out_ptrs, const float* const* src_ptrs,
                                       const int32_t* csr_ptr, const int32_t* csr_idx,
                                       const double* csr_coef, int D, size_t P, int mode, size_t cbegin,
                                       size_t cend, unsigned long long* kept_counts, void* stream);

/* (f4) Scheduled population round: cfa_mix_population_f32 under a topology that changes from
 * round to round (cfa_mobilenet.py:136-138 takes each epoch's neighbours from vGraph.mat,
 * cfa_ongraphs.py:33-52 redraws them at every call) with no host work between rounds.
 * csr_ptr holds T tables of D + 1 row offsets back to back (table t = csr_ptr + t * (D + 1)); the
 * offsets are ABSOLUTE positions in the csr_idx / csr_coef all tables share. sched is a DEVICE
 * array of S table indices, each in [0, T) (device memory: not checked here, the caller checks
 * them before the upload), and round a DEVICE word, the round counter. A call mixes every device
 * with table sched[*round mod S] and leaves *round one higher, in stream order (a one-lane launch
 * after the mix, so every workgroup of the round reads the same value). The kernel finds its
 * table itself: a captured sequence of calls replays any number of times, each replayed call
 * with its own round's table. Rules, the < 4-element tail and the D <= 65535 limit as
 * cfa_mix_population_f32. S <= 0, T <= 0 or a null sched / round: CFA_E_INVALID. D == 0 or
 * P == 0: CFA_OK, and the counter is NOT advanced (no round was mixed). */
CFA_API int cfa_mix_population_sched_f32(float* const* out_ptrs, const float* const* src_ptrs,
                                         const int32_t* csr_ptr, const int32_t* csr_idx,
                                         const float* csr_coef, const int32_t* sched, int S, int T,
                                         unsigned long long* round, int D, int rule, size_t P,
                                         void* stream);

/* (f4) The same for cfa_mix_population_tf1_f32: its numerics, its compression epilogue and its
 * kept_counts (zeroed by the caller before every call), with the table of the round as above
 * (csr_coef DEVICE double, shared by all tables). D == 0 or P == 0: CFA_OK, counter not advanced. */
CFA_API int cfa_mix_population_sched_tf1_f32(float* const* out_ptrs, const float* const* src_ptrs,
                                             const int32_t* csr_ptr, const int32_t* csr_idx,
                                             const double* csr_coef, const int32_t* sched, int S, int T,
                                             unsigned long long* round, int D, size_t P, int mode,
                                             size_t cbegin, size_t cend, unsigned long long* kept_counts,
                                             void* stream);

/* (a5/a6 batched) Population round with the TF2 protocol's training_end rule, the flags on the
 * device: cfa_mix_population_f32 (CFA_RULE_SEQUENTIAL, the same CSR layout, the same three
 * roundings per step) where nobody has ended, and with no host work between rounds where somebody
 * has. ended [D] (DEVICE int32, the round's input): device d has reported training_end. Per device:
 *   ended[d] != 0: out[d] is a bit copy of its own row (it has left its loop,
 *       federated_learning_keras_consensus_FL_threads_MNIST.py:501-546), saw[d] = 0.
 *   otherwise the device collects its list in order and stops after the first flagged neighbour,
 *   at list position f (consensus_v3.py:139-141; consensus_v4.py:191-193, :234-236):
 *     CFA_ENDED_COPY, f found: out[d] is a bit copy of that neighbour's row, loaded and stored
 *         with no arithmetic (consensus_v3.py:147-152, consensus_v4.py:205-210).
 *     CFA_ENDED_TRUNCATE, f found: the fold of positions 0..f with the table's coefficients
 *         (consensus_v4.py:248: the caller's eps).
 *     CFA_ENDED_TRUNCATE_EPS, f found or not: the fold of m positions, m = f + 1 or the whole
 *         list, every step with (float)(1.0 / (double)(m + 1)) (consensus_v3.py:233, as numpy
 *         applies the Python float to fp32 arrays).
 *     COPY and TRUNCATE without a flagged neighbour: the table's mix, as cfa_mix_population_f32.
 *   saw[d] = 1 if a flagged neighbour was found, else 0 (getTrainingStatusFromNeightbor());
 *   ended_next[d] = ended[d] | saw[d]. Both are DEVICE int32 [D] or NULL, and must not overlap
 *   ended: the launch reads only ended and writes these two.
 * sched == NULL and round == NULL: one table (S and T unused). Otherwise both are given and the
 * call is scheduled as cfa_mix_population_sched_f32: table sched[*round mod S], *round left one
 * higher in stream order. CFA_E_INVALID: an unknown ended_rule, a null ended, ended_next or saw
 * overlapping ended, a null table, D < 0 or D > 65535, sched without round or round without sched,
 * S <= 0 or T <= 0 under a schedule. D == 0 or P == 0: CFA_OK, and the counter is NOT advanced. */
CFA_API int cfa_mix_population_ended_f32(float* const* out_ptrs, const float* const* src_ptrs,
                                         const int32_t* csr_ptr, const int32_t* csr_idx,
                                         const float* csr_coef, const int32_t* sched, int S, int T,
                                         unsigned long long* round, const int32_t* ended,
                                         int32_t* ended_next, int32_t* saw, int ended_rule, int D,
                                         size_t P, void* stream);

/* (f1 batched) FedAvg parameter-server round on a device-resident population, one launch per
 * round: the server's fold of the round's active devices into the global model, then every
 * device's take of the published model, with no host work between rounds.
 *   models  [D, pitch] fp32 rows (DEVICE), row d = device d's model, updated in place by the client
 *           rule. Rows start 16-byte aligned (base aligned, pitch a multiple of 4 elements);
 *           P <= pitch may be any size: the last P mod 4 elements take a scalar tail in the same
 *           launch. Columns P .. pitch-1 are never touched.
 *   params  [P] fp32 (DEVICE, 16-byte aligned), the global model, updated in place.
 *   act_ptr [T + 1], act_idx: T active lists back to back (DEVICE); list t is act_idx[act_ptr[t] ..
 *           act_ptr[t + 1]), device ids in fold order, duplicates allowed (the reference folds a
 *           list: parameter_server_v2.py:88, active_devices = indexes_tx[:, epoch]). The ids are
 *           device memory: not checked here, the caller checks them before the upload.
 *   act_div [T] float C of each list and act_rdiv [T] double RN_64(1 / C) (DEVICE), built by the
 *           caller as 1.0 / (double)act_div[t]: the kernel forms no reciprocal itself.
 *   sched [S], round: as cfa_mix_population_sched_f32. The call uses list sched[*round mod S] and
 *           leaves *round one higher, in stream order.
 *   ended   [D] int32 flags (DEVICE), or NULL: device d reported training_end.
 * Server (parameter_server_v2.py:146-161, parameter_server.py:154, PS_server.py:130-133): for the
 * C entries k of the round's list in order, p <- p + (u * (x_k - p)) / C, every operation rounded
 * to fp32 as numpy does (the CFA_RULE_SEQUENTIAL_DIV step, identical to cfa_mix_seq_div_f32 bit for
 * bit, exact subnormal ties included). If any entry of the list is flagged in `ended`, the server
 * instead takes the transfer-learning step p <- p + u * (x_e - p) on the FIRST flagged entry in
 * list order, with no division, and folds nothing else (:150-157). An empty list leaves params
 * unchanged; the client rule still runs.
 * Client: CFA_CLIENT_NONE writes params only; CFA_CLIENT_COPY makes every row the new params
 * (federated_learning_keras_PS_MNIST.py:307-309); CFA_CLIENT_MIX gives every row
 * w <- w + (u_c * (g - w)) / d_c with g the new params and rd_c = RN_64(1 / d_c)
 * (learner_consensus.py:151-152; d_c = 1 divides exactly: a plain w + u_c * (g - w) client).
 * Rows of devices that were not active are updated too. Each lane owns its columns for the whole
 * round (it reads and writes a given element of params and of every row itself), so the update is
 * in place with no second stack.
 * CFA_E_INVALID: a null table, S <= 0 or T <= 0, D < 0, pitch < P, an unknown client rule,
 * d_c == 0 under CFA_CLIENT_MIX. CFA_E_UNSUPPORTED: a base or pitch that is not 16-byte aligned.
 * P == 0: CFA_OK, and the counter is NOT advanced. */
CFA_API int cfa_fedavg_population_round_f32(float* models, size_t pitch, float* params,
                                            const int32_t* act_ptr, const int32_t* act_idx,
                                            const float* act_div, const double* act_rdiv, float u,
                                            const int32_t* sched, int S, int T,
                                            unsigned long long* round, const int32_t* ended,
                                            int client, float u_c, float d_c, double rd_c, int D,
                                            size_t P, void* stream);

/* (f1 batched, TF1) One server-federation epoch of the CFA-FA driver on a device-resident
 * population, one launch: the server's fold of the D published models into its fp64 model, then
 * every device's pull toward it (federated_sample_CNN_CFA_FA.py; the per-model host form is
 * federated_amd.server.cfa_fa_server_init / _round / cfa_fa_client_mix over cfa_fold_f64).
 *   in   [D, in_pitch] fp32 rows (DEVICE), row d = the model device d trained and published at
 *        this epoch (cfa.py:146-153 with consensus disabled). Only read.
 *   out  [D, out_pitch] fp32 rows (DEVICE), row d = device d's model after the epoch. Must not
 *        overlap `in`. Columns P .. pitch-1 of either stack are never touched.
 *   s    [P] fp64 (DEVICE), the server model, updated in place.
 *   coef [D] fp64 (DEVICE): b_d under CFA_FA_INIT, the one fp64 product eps * b_d under
 *        CFA_FA_ROUND, formed by the caller as the driver forms it.
 * CFA_FA_INIT (:73-89): for d = 0 .. D-1 in order, s <- s + coef[d] * x_d; out row d = in row d.
 * CFA_FA_ROUND (:103-110, :130-133, then :280-283): for d in order, s <- s + coef[d] * (x_d - s);
 * then with that final s every row W = in row d gives out row d = (float)(W + eps2 * (s - W)).
 * x_d and W are widened exactly; every product and sum is one fp64 operation with its own rounding
 * (no FMA), the client result is rounded once to fp32: numpy's values bit for bit, identical on
 * every run and under graph replay (a lane owns its columns; no atomics, no workspace, nothing
 * queried or allocated at launch).
 * Rows and s may have any alignment their element types allow: when every base is 16-byte aligned
 * and both pitches are multiples of 4 the rows go as float4 and s as double2, anything else
 * element by element with the same results. With D above the load batch (8, or 4 under
 * CFA_FA_BATCH=4) the D input rows are read twice, once per step; s and coef once.
 * CFA_E_INVALID: a null pointer, D < 0, a pitch below P, an unknown mode, `out` overlapping `in`.
 * P == 0: CFA_OK, nothing launched. D == 0: s is left unchanged. */
CFA_API int cfa_fa_population_round_f32(float* out, size_t out_pitch, const float* in, size_t in_pitch,
                                        double* s, const double* coef, double eps2, int mode, int D,
                                        size_t P, void* stream);
/* Elements of one workgroup's tile of that launch for rows of P elements (aligned: the float4
 * form; else the element form): where its grid-stride loop and its partial tile begin. */
CFA_API size_t cfa_fa_round_tile(size_t P, int aligned);

/* (a4 batched) CFA-GE population step: stage 1 and the gradient step of every device of a
 * device-resident population in one launch (cfa_ge_2stage.py:446-466, then :591-621). For device
 * d, CSR entries e in [csr_ptr[d], csr_ptr[d+1]): the first is its local model
 * src_ptrs[csr_idx[e0]], the others its neighbours in order, mixed with the sequential rule and
 * coefficient csr_coef[e]; then for each neighbour entry e, in order:
 *   s <- rho * g + (1 - rho) * s   (s = state_ptrs[e], g = grad_ptrs[e], NULL = zero gradient)
 *   w <- w - lr(i) * (use_filtered ? s : g),   lr(i) = i < lr_split ? lr1 : lr2
 * and out_ptrs[d] = w. Every table is a DEVICE array; entry e0's state/grad slots are unused.
 * Same operations, same order, same results as cfa_mix_population_f32 + cfa_mewma_update_f32.
 * reduce_ws != NULL: the same launch also sums the reduce_splits partial buckets of reduce_M
 * gradient evaluations (reduce_ws [reduce_M][reduce_splits][P], from a partials-only
 * cfa_ge_grad_*_rows_f32) into reduce_out [reduce_M][P], in split order: the same sums as the
 * rows launch's own reduction. A CFA-GE round is then two launches: the gradients of this round
 * (partials), and this step (previous round's gradients) + this round's reduction.
 * reduce_out must not alias any table or bucket the step reads. */
CFA_API int cfa_ge_population_step_f32(float* const* out_ptrs, const float* const* src_ptrs,
                                       float* const* state_ptrs, const float* const* grad_ptrs,
                                       const int32_t* csr_ptr, const int32_t* csr_idx,
                                       const float* csr_coef, int D, double rho, float lr1, float lr2,
                                       size_t lr_split, int use_filtered, size_t P,
                                       const float* reduce_ws, float* reduce_out, int reduce_M,
                                       int reduce_splits, void* stream);

/* ---------------------------------------------------------------------------------------
 * Multi-GPU (RCCL over xGMI): one process per GPU.
 * The reference has no collectives; its cross-device edges are files polled on a shared
 * directory (TF1/consensus/cfa.py:119-130, TF2 consensus_v3.py:82-141). When the simulated
 * population is sharded over the GPUs of one node those edges become RCCL transfers.
 */
#define CFA_UNIQUE_ID_BYTES 128

/* Fill `id` (CFA_UNIQUE_ID_BYTES bytes) on one rank; share it with the others out of band. */
/* The RCCL library version libcfa runs on (ncclGetVersion), for the record of a multi-GPU run. */
CFA_API int cfa_rccl_version(int* version);
CFA_API int cfa_comm_unique_id(void* id);
/* Create a communicator for `rank` of `nranks` on HIP device `device`. */
CFA_API int cfa_comm_init(void** comm, int rank, int nranks, const void* id, int device);
CFA_API int cfa_comm_destroy(void* comm);
/* Grouped point-to-point halo exchange of whole buckets: send_bufs[i] (P floats) goes to
 * rank send_peers[i], recv_bufs[i] is filled from recv_peers[i]. One RCCL group. */
CFA_API int cfa_halo_exchange_f32(void* comm, const float* const* send_bufs, const int* send_peers,
                          int nsend, float* const* recv_bufs, const int* recv_peers, int nrecv,
                          size_t P, void* stream);
/* Grouped point-to-point exchange of element ranges with per-message lengths: send_bufs[i]
 * (send_counts[i] floats) goes to rank send_peers[i]; recv_bufs[i] (recv_counts[i] floats) is
 * filled from recv_peers[i]. One RCCL group; messages between one rank pair pair up in issue
 * order. This is the step of the routed (multi-link, relayed) halo exchange: a group carries
 * the direct pieces and first relay hops of one stage and the second hops of the previous one
 * (federated_amd/halo.py). Zero-length messages are skipped on both sides. Replaces the same
 * file polling as cfa_halo_exchange_f32 (TF1/consensus/cfa.py:119-130). */
CFA_API int cfa_p2p_group_f32(void* comm, const float* const* send_bufs, const size_t* send_counts,
                      const int* send_peers, int nsend, float* const* recv_bufs,
                      const size_t* recv_counts, const int* recv_peers, int nrecv, void* stream);
/* Sum all-reduce / reduce of pre-scaled buckets (FedAvg / parameter-split sums). */
CFA_API int cfa_allreduce_sum_f32(void* comm, const float* send, float* recv, size_t count,
                          void* stream);
CFA_API int cfa_reduce_sum_f32(void* comm, const float* send, float* recv, size_t count, int root,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * (f2) Host-resident buckets without staging copies. Device address of a pinned host buffer
 * (hipHostMalloc, torch pin_memory). Passing it to the mix entry points makes the kernel read
 * its buckets over PCIe and write the result straight into host memory: no H2D/D2H staging,
 * and the link's two directions are busy at once. Replaces the staging copies around the mix
 * when buckets arrive in host memory: TF1/consensus/cfa.py:108-117 (.mat loads),
 * TF2 FL_threads_CIFAR100.py:424-428 (.npy), FL_over_MQTT/learner_consensus.py:136-145.
 * Fails (CFA_E_HIP) for memory the runtime has not mapped for the device.
 */
CFA_API int cfa_host_device_pointer(const void* host, void** dev);

/* ---------------------------------------------------------------------------------------
 * (f2) MQTT model payloads, host side. FL_over_MQTT ships models as
 *   pickle.dumps({'model_layer{k}': w_k.tolist(), 'device': i, 'framecount': f,
 *                 'local_epoch': e, 'training_end': b})
 * (TF2/FL_over_MQTT/learner_consensus.py:257-268; PS_server.py:137-149 answers with
 * 'global_model_layer{k}', 'global_epoch', 'training_end') and decodes them with
 * pickle.loads + np.asarray (learner_consensus.py:136-144, PS_server.py:90-118).
 * The codec below reads and writes those bytes without Python objects:
 *   - decode: one structure pass over the payload, then the float runs of a key are
 *     byte-swapped straight into a caller buffer (e.g. a pinned staging bucket), threaded for
 *     large tensors. Values equal np.asarray(pickle.loads(payload)[key]) bit for bit (fp64), or
 *     that array cast to fp32 (`_f32`). Only dict/list/str/int/bool/float/None and memo opcodes
 *     are accepted; object-constructing opcodes (GLOBAL, REDUCE, BUILD, ...) are refused, so a
 *     payload executes nothing. `buf` must stay alive and unchanged until cfa_payload_free.
 *   - encode: the exact bytes of pickle.dumps(d, protocol) (CPython 3.10, framing included)
 *     for d = {key: ndarray.tolist() | int | bool | float | None} in item order.
 */
typedef struct cfa_payload cfa_payload_t;  /* opaque parsed payload */
#define CFA_PAYLOAD_MAX_DIM 8
enum {
  CFA_PAYLOAD_NONE = 0,
  CFA_PAYLOAD_BOOL = 1,
  CFA_PAYLOAD_INT = 2,
  CFA_PAYLOAD_FLOAT = 3,
  CFA_PAYLOAD_F32_ARRAY = 4,   /* encode only: float32 data, tolist() values */
  CFA_PAYLOAD_F64_ARRAY = 5,   /* (nested) list whose np.asarray dtype is float64 */
  CFA_PAYLOAD_I64_ARRAY = 6,   /* decode only: list of ints (np.asarray -> int64) */
  CFA_PAYLOAD_BOOL_ARRAY = 7,  /* decode only: list of bools */
  CFA_PAYLOAD_STR = 8,         /* decode only */
  CFA_PAYLOAD_DICT = 9         /* decode only (nested dict; not readable as an array) */
};
typedef struct {
  const char* key;       /* NUL-terminated UTF-8 */
  int kind;              /* CFA_PAYLOAD_NONE .. CFA_PAYLOAD_F64_ARRAY */
  const void* data;      /* arrays: C-contiguous host data of `shape` */
  int ndim;              /* arrays: 0 .. CFA_PAYLOAD_MAX_DIM (0 = one float, as tolist()) */
  const int64_t* shape;  /* arrays: ndim extents */
  int64_t ivalue;        /* INT / BOOL */
  double fvalue;         /* FLOAT */
} cfa_payload_item_t;

CFA_API int cfa_payload_parse(const void* buf, size_t len, cfa_payload_t** out);
CFA_API void cfa_payload_free(cfa_payload_t* payload);
/* Number of top-level keys; negative CFA_E* on error. */
CFA_API int cfa_payload_num_keys(const cfa_payload_t* payload);
/* Key `index` (insertion order) as a pointer into the payload bytes (not NUL-terminated). */
CFA_API int cfa_payload_key(const cfa_payload_t* payload, int index, const char** key, size_t* len);
/* Kind, shape (up to CFA_PAYLOAD_MAX_DIM extents) and element count of `key`'s value. */
CFA_API int cfa_payload_info(const cfa_payload_t* payload, const char* key, int* kind, int* ndim,
                             int64_t* shape, int64_t* numel);
/* A scalar value (None / bool / int / float): ivalue for bool and int, fvalue for all. */
CFA_API int cfa_payload_scalar(const cfa_payload_t* payload, const char* key, int* kind,
                               int64_t* ivalue, double* fvalue);
/* Row-major values of `key` (numel must match) into host memory. */
CFA_API int cfa_payload_read_f64(const cfa_payload_t* payload, const char* key, double* dst,
                                 int64_t numel);
CFA_API int cfa_payload_read_f32(const cfa_payload_t* payload, const char* key, float* dst,
                                 int64_t numel);
/* Encode n items with pickle protocol 2..5. dst == NULL: only *size is set (the exact length).
 * Otherwise dst must hold cap >= *size bytes (CFA_E_INVALID if not; *size is still set). */
CFA_API int cfa_payload_encode(const cfa_payload_item_t* items, int n, int protocol, void* dst,
                               size_t cap, size_t* size);

#ifdef __cplusplus
}
#endif
#endif /* CFA_ENGINE_H */

// Native orchestration of the ResNet18 TripletNet(_Finetune)+head graph: forward (eval-folded or train-mode BN),
// backward, gradient all-reduce (RCCL, bucketed + overlapped), synced BatchNorm, fused optimizer.  One C call per
// step; every kernel goes to the caller's stream.  See include/sslcr.h for the reference code each entry replaces.
#include <rccl/rccl.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <vector>

#include "kernels.hpp"

using namespace sslcr;

#define TRY(expr)                                   \
  do {                                              \
    hipError_t _e = (expr);                         \
    if (_e != hipSuccess) return check(_e, #expr);  \
  } while (0)
#define TRYI(expr)            \
  do {                        \
    int _r = (expr);          \
    if (_r != 0) return _r;   \
  } while (0)
#define TRYN(expr)                                                                     \
  do {                                                                                 \
    ncclResult_t _r = (expr);                                                          \
    if (_r != ncclSuccess) return fail("%s: %s", #expr, ncclGetErrorString(_r));       \
  } while (0)

namespace {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    if (p) {
      hipError_t e = hipFree(p);          // synchronises the device: only ever happens while shapes grow
      if (e != hipSuccess) return check(e, "hipFree");
      p = nullptr;
      cap = 0;
    }
    bytes = (bytes + 255) & ~(size_t)255;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return check(e, "hipMalloc");
    cap = bytes;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct Carver {                 // bump allocator over a DevBuf region (offsets only; ensure() afterwards)
  size_t off = 0;
  size_t take(size_t bytes) {
    size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  }
};

struct ConvL {
  int cin = 0, cout = 0, k = 0, stride = 1, pad = 0, pidx = -1;
  void *w_fwd = nullptr, *w_dg = nullptr, *w_fold = nullptr;
  float* b_fold = nullptr;
  // bf16 storage: the eval pack keeps the PLAIN filter and the BatchNorm scale goes to the conv's epilogue (sslcr_conv_desc.out_scale):
  // the loss error of the full-size iteration is 3.6 x smaller than with the scale folded in before the rounding; nullptr (fp32
  // mode): folded into w_fold
  float* s_fold = nullptr;
  void* w_foldf = nullptr;        // stem only, with s_fold: the FOLDED eval pack for the shapes the fused conv + max-pool kernel does not take
                                  // (stem_fwd_kernel has no output scale: its registers, see launch_stem)
  // fp8 engine mode (SSLCR_FP8): e4m3 shadow packs + per-kout dequant factors of the train / eval-folded filters, for the
  // convs the fp8 kernel serves (3x3 stride 1, cin and cout multiples of 128: layers 2-4)
  uint8_t *w8_fwd = nullptr, *w8_fold = nullptr;
  float *dq_fwd = nullptr, *dq_fold = nullptr;
  float* f8s = nullptr;     // delayed activation scaling: {x_scale, amax} of the train forward, {x_scale, amax} of the eval forward
};
struct BnL {
  int C = 0, pg = -1, pb = -1, bidx = -1;
};
struct BlockL {
  ConvL c1, c2, ds;
  BnL b1, b2, bd;
  bool has_ds = false;
  int pstart = 0;
};
struct Layer {                  // a conv and the BatchNorm behind it
  ConvL* conv;
  BnL* bn;
};
constexpr int kLayers = 20;     // the stem, two convs per block, three projections
struct BnSaved {
  float *scale, *shift, *mean, *invstd;
};
struct PassState {
  const void* x = nullptr;
  const void* x2 = nullptr;      // second input segment (images n >= n_split), see sslcr_stem_desc
  int n_split = 0;
  int in_f32 = 0, N = 0, H = 0, W = 0;
  DevBuf mem;
  char* raw0 = nullptr;
  char* pooled = nullptr;
  uint8_t* argmax = nullptr;
  struct {
    char *raw1, *raw2, *rawd, *y;
    uint8_t* ybits;              // bf16 mode: one bit per element of y, (y > 0) -- what bn2's backward reduce pass reads instead of y
  } blk[8];
  BnSaved bn[20];
  float* E = nullptr;
};

}  // namespace

struct ProfRec {
  hipEvent_t e0, e1;
  double flops, bytes;
  const char* name;       // the kernel template instance that was launched
};
struct Profiler {               // optional HIP-event bracketing of the conv launches (bench.py roofline leg)
  bool on = false;
  std::vector<ProfRec> rec[3];  // 0: conv (fwd + dgrad), 1: wgrad, 2: bn_bwd_apply (the largest HBM-bound kernel; flops = 0)
  std::vector<hipEvent_t> pool;
  hipEvent_t get() {
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
};

// "Virtual ranks": W engine contexts of ONE process on ONE device (one host thread and one stream each) exchange through this
// object instead of RCCL -- every sharded code path of the engine (synced BatchNorm forward/backward sums, global-count loss
// scaling, bucketed gradient sums on the side stream) then runs with world = W on a single-GPU box and can be compared with the
// 1-rank step on the concatenated batch (tests/test_engine_gpu2.py).  RCCL refuses two ranks on one device, hence the stand-in;
// it is deterministic (ranks summed in rank order) and asynchronous on the callers' streams like the real collective.
constexpr int VW_MAX = 8;
struct VChan {                      // one per collective stream (0: BatchNorm sums on the compute streams, 1: gradient buckets)
  std::mutex m;
  std::condition_variable cv;
  int arrived = 0;
  long gen = 0;
  void* slot[2][VW_MAX] = {};       // [call parity][rank]: that rank's contribution, device memory owned by the rank
  size_t cap[2][VW_MAX] = {};
  hipEvent_t ev_in[2][VW_MAX] = {}, ev_out[2][VW_MAX] = {};
  bool out_set[2][VW_MAX] = {};
  long calls[VW_MAX] = {};
};
struct sslcr_vcomm {
  int world = 1;
  VChan ch[2];
  std::atomic<bool> poisoned{false};   // a rank timed out inside a collective: its call parity is out of step with its peers for good
};

struct sslcr_ctx {
  Profiler prof;
  int device = 0, dtype = 0;
  int fp8 = 0;                    // SSLCR_FP8: dtype stays bf16 (storage, backward); eligible forward convs run the e4m3 kernel
  sslcr_vcomm* vcomm = nullptr;   // set instead of comm / comm_g by sslcr_comm_init_virtual
  ncclComm_t comm = nullptr;      // BatchNorm-sum all-reduces, only ever used on the caller's (compute) stream
  ncclComm_t comm_g = nullptr;    // gradient buckets, only ever used on comm_stream (one communicator per stream, like
                                  // separate process groups: no cross-stream serialisation inside RCCL)
  int rank = 0, world = 1;
  int bn_sync = 1;                // train-mode BatchNorm on GLOBAL batch statistics (all-reduce of per-channel sums); 0 = per replica
  hipStream_t comm_stream = nullptr;
  // second compute stream: the (frozen, eval-mode) teacher forward of an SSL_CR step runs next to the student forward, so the
  // workgroups of one fill the tail rounds of the other's persistent kernels (the two share no buffers: the teacher works in
  // ctx scratch, which the student only touches in backward)
  hipStream_t aux_stream = nullptr;
  hipEvent_t ev_aux_begin = nullptr, ev_aux_end = nullptr;
  int use_aux = 0;                // sslcr_set_aux_stream
  // weight-gradient side stream: in backward the wgrad launches (MFMA-bound, 3 ms of the step) depend only on a BatchNorm-backward
  // output and feed nothing but the gradient buffer, while the chain they leave behind alternates MFMA-bound dgrads with
  // HBM-bound BatchNorm passes (2.4 ms) that leave the matrix pipes idle -- so they are launched on a second stream behind an
  // event and fill those gaps.  kinds: 0 = a block's conv2 (reads the dRaw2 scratch), 1 = conv1 (dRaw1), 2 = projection (dRawD);
  // ev_wg_done[k] orders the NEXT writer of that scratch buffer behind the reader.
  hipStream_t wg_stream = nullptr;
  hipEvent_t ev_wg_in[3] = {nullptr, nullptr, nullptr}, ev_wg_done[3] = {nullptr, nullptr, nullptr}, ev_wg_join = nullptr;
  bool wg_pending[3] = {false, false, false};
  bool wg_any = false;            // something was launched on wg_stream since the last join
  int fuse_stem_bwd = 1;          // conv1 wgrad derives dY from the pooled gradient in LDS (SSLCR_FUSE_STEM_BWD=0: apply pass + wgrad, for A/B runs)
  int use_wg = 0;                 // sslcr_set_wgrad_stream (default off: measured neutral, see include/sslcr.h; off while profiling)
  hipEvent_t ev_ready[8], ev_done = nullptr;
  DevBuf scratch;     // eval-forward activations and backward transients (never live at the same time)
  DevBuf partials;    // BN partial rows
  DevBuf small;       // bn stage/sums, unit scale/shift
  double* bn_stage = nullptr;
  double* bn_sums = nullptr;
  int* bn_tickets = nullptr;      // sslcr_bn_finalize_desc.tickets: 16 zeroed ints (every BatchNorm finalize of this context runs on one stream at a time)
  // BatchNorm-backward sums: every reduce pass of one backward takes its own [2][2][512]-double slot of this ring (the pass
  // overwrites it with the ordered sum of its workgroups' rows: nothing to clear)
  DevBuf bn_ring;
  int bn_ring_i = 0;
  static constexpr int kBnRing = 96, kBnSlot = 2 * 2 * 512;
  float *ones = nullptr, *zeros = nullptr;
  size_t esz() const { return dtype == DT_BF16 ? 2 : 4; }
};

struct sslcr_net {
  sslcr_ctx* ctx = nullptr;
  const void* split_x2 = nullptr;   // set by sslcr_step_ssl_cr around the student pass: input = (x[0:split_n], split_x2)
  int split_n = 0;
  int nparams = 0, head_kind = 0, ncls = 1, triplet = 0;
  std::vector<float*> params;
  std::vector<uint8_t> rg;
  std::vector<int> psize;
  std::vector<size_t> goff;
  float* bn_rm[20];
  float* bn_rv[20];
  int64_t* bn_nbt[20];
  ConvL stem;
  BnL bn0;
  BlockL blocks[8];
  // every conv with its BatchNorm in parameter order (index = BnL::bidx): THE walk over the net's layers (build_topology fills it) ...
  Layer layers[kLayers];
  // ... and parameter -> block conv (nullptr: the stem, whose pack has its own K order, a BatchNorm or a head parameter)
  std::vector<const ConvL*> block_conv;
  DevBuf shadow, grads, heads, descs, chunks, f8buf;
  DevBuf norm_ws;     // gradient norm: GRAD_NORM_BLOCKS double partials, then {norm, coef}
  float* f8slots = nullptr;       // [n8][2] = {x_scale, amax since the last update}: two slots (train, eval) per fp8 conv, see ConvL::f8s
  int n8 = 0;
  bool f8_cal[2] = {false, false};  // the first forward of this net in (train, eval) mode has calibrated the activation scales
  bool f8_calib_pass = false;       // a calibration pass is running: no running-statistics update, outputs discarded
  int nchunks = 0;
  bool opt_packs_all = false;     // the optimizer work list rewrites every non-stem conv's train-mode shadow weights
  size_t grad_count = 0;
  // gradient accumulation (sslcr_net_set_grad_accumulate): gw is where a backward WRITES -- grads.p, or gnew.p while an accumulating
  // backward runs, whose sum into grads follows the joins at the end of net_backward.  Everything that reads gradients reads grads.
  DevBuf gnew;
  float* gw = nullptr;
  bool grad_accum = false, had_backward = false;
  LossOpts lopts = loss_opts_default();      // sslcr_net_set_loss_opts: the loss leg of the step entries (defaults: launch_loss itself)
  PassState pass[3];
  bool ybits_ok = false;         // the passes' mask bits are allocated back to back (what the segment forms assume)
  // heads state (fp32)
  int hN = 0;
  float *cat[3], *hact[3], *fi[3], *feats = nullptr, *hid = nullptr, *logits = nullptr, *dE[3], *dfeats = nullptr, *dhid = nullptr,
        *dtmp256 = nullptr, *dtmp512 = nullptr, *dcat = nullptr, *scratch = nullptr, *dlogits = nullptr, *logits_t = nullptr;
  int last_N = 0, last_npass = 0;
  bool last_segments = false;      // the last train forward ran the branches as segments
  bool packed_train = false, packed_eval = false;
  // sslcr_net_debug_tap: backward keeps copies of each block's transient gradient tensors, per pass, for the layer-wise replay test
  bool tap = false;
  static constexpr int kTapSlots = 7;
  DevBuf tapbuf[3][8][kTapSlots];
  int tapdims[3][8][kTapSlots][4] = {};
  // which form each stage of the block took (include/sslcr.h: sslcr_net_debug_tensor's flags).  Backward bits: 0 dAct1 was written
  // with bn1's ReLU mask already applied, 1 seg_bn, 2 seg_dg, 3 c2_batched, 4 paired BatchNorm backward, 5 par4 in one launch;
  // fwd_flags: 6 the forward ran as segments, 7 BlockPlan::paired.  Written by every step, read by the tap only
  int tap_flags[8] = {};
  int fwd_flags[8] = {};
  std::vector<sslcr_tensor_desc> host_descs;
  std::vector<float*> st1, st2;
  std::vector<int> group_of;      // parameter -> optimizer group of the descriptor table in `descs`
  int ndesc = 0, max_n = 0;
  // every device buffer the net owns (a new DevBuf member is added here, nowhere else): what sslcr_net_destroy releases
  std::vector<DevBuf*> bufs() {
    std::vector<DevBuf*> v = {&shadow, &grads, &gnew, &heads, &descs, &chunks, &f8buf, &norm_ws};
    for (PassState& ps : pass) v.push_back(&ps.mem);
    for (auto& ps : tapbuf)
      for (auto& row : ps)
        for (DevBuf& b : row) v.push_back(&b);
    return v;
  }
};

namespace {

struct VSrc { const void* p[VW_MAX]; };
template <typename T>
__global__ void vsum_kernel(T* dst, VSrc src, int W, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    T s = static_cast<const T*>(src.p[0])[i];
    for (int q = 1; q < W; ++q) s += static_cast<const T*>(src.p[q])[i];       // rank order: every rank gets the same bits
    dst[i] = s;
  }
}

std::atomic<int> g_live_ctx{0};     // contexts between sslcr_create and sslcr_destroy (see sslcr_destroy)

inline bool sharded(const sslcr_ctx* c) { return c->comm != nullptr || c->vcomm != nullptr; }

int vcomm_all_reduce(sslcr_ctx* c, int chan, void* buf, size_t count, bool f64, hipStream_t st) {
  sslcr_vcomm* v = c->vcomm;
  VChan& ch = v->ch[chan];
  const int r = c->rank, W = v->world;
  const size_t bytes = count * (f64 ? 8 : 4);
  if (v->poisoned) return fail("virtual all-reduce: the communicator was poisoned by an earlier timeout");
  const int ph = (int)(ch.calls[r]++ & 1);
  // the slot is reused every second call: its previous readers (the peers' sum kernels of two calls ago) recorded ev_out then
  for (int q = 0; q < W; ++q)
    if (q != r && ch.out_set[ph][q]) TRY(hipStreamWaitEvent(st, ch.ev_out[ph][q], 0));
  if (ch.cap[ph][r] < bytes) {
    if (ch.slot[ph][r]) TRY(hipFree(ch.slot[ph][r]));       // (synchronises the device)
    ch.slot[ph][r] = nullptr; ch.cap[ph][r] = 0;
    TRY(hipMalloc(&ch.slot[ph][r], (bytes + 255) & ~(size_t)255));
    ch.cap[ph][r] = (bytes + 255) & ~(size_t)255;
  }
  if (!ch.ev_in[ph][r]) {
    TRY(hipEventCreateWithFlags(&ch.ev_in[ph][r], hipEventDisableTiming));
    TRY(hipEventCreateWithFlags(&ch.ev_out[ph][r], hipEventDisableTiming));
  }
  TRY(hipMemcpyAsync(ch.slot[ph][r], buf, bytes, hipMemcpyDeviceToDevice, st));
  TRY(hipEventRecord(ch.ev_in[ph][r], st));
  {                                                   // host rendezvous: every rank has published its slot and event
    std::unique_lock<std::mutex> lk(ch.m);
    const long g = ch.gen;
    if (++ch.arrived == W) {
      ch.arrived = 0; ++ch.gen;
      ch.cv.notify_all();
    } else if (!ch.cv.wait_for(lk, std::chrono::seconds(120), [&] { return ch.gen != g; })) {
      --ch.arrived;
      c->vcomm->poisoned = true;          // calls[r] and the slot are already published: every later collective would pair up wrongly
      ch.cv.notify_all();
      return fail("virtual all-reduce: rank %d waited 120 s for its peers (channel %d); the communicator is now unusable", r, chan);
    }
  }
  VSrc src;
  for (int q = 0; q < W; ++q) {
    src.p[q] = ch.slot[ph][q];
    if (q != r) TRY(hipStreamWaitEvent(st, ch.ev_in[ph][q], 0));
  }
  const int blocks = (int)((count + 255) / 256 < 1024 ? (count + 255) / 256 : 1024);
  if (f64) hipLaunchKernelGGL(vsum_kernel<double>, dim3(blocks), dim3(256), 0, st, (double*)buf, src, W, count);
  else hipLaunchKernelGGL(vsum_kernel<float>, dim3(blocks), dim3(256), 0, st, (float*)buf, src, W, count);
  TRY(hipGetLastError());
  TRY(hipEventRecord(ch.ev_out[ph][r], st));
  ch.out_set[ph][r] = true;
  return 0;
}

// SUM all-reduce in place over the ranks of this job: channel 0 = BatchNorm sums (compute stream), 1 = gradient buckets (side stream)
int all_reduce(sslcr_ctx* c, int chan, void* buf, size_t count, bool f64, hipStream_t st) {
  if (c->vcomm) return vcomm_all_reduce(c, chan, buf, count, f64, st);
  TRYN(ncclAllReduce(buf, buf, count, f64 ? ncclDouble : ncclFloat, ncclSum, chan == 0 ? c->comm : c->comm_g, st));
  return 0;
}

// ---- launch wrappers.  The one profiling bracket: with the profiler off it is launch() and nothing else; with it on, two HIP events
// around the launch on ITS stream and a record in rec[slot] (see Profiler).  `book` fills the record's name / flops / bytes -- the
// algorithmic work (forward-conv FLOPs even for the strided dgrad gather, whose zero taps are not counted) -- and only runs when profiling
template <class Book, class Launch>
hipError_t profiled(sslcr_ctx* c, int slot, hipStream_t st, Book&& book, Launch&& launch) {
  if (!c->prof.on) return launch();
  ProfRec r;
  r.e0 = c->prof.get(); r.e1 = c->prof.get();
  book(r);
  (void)hipEventRecord(r.e0, st);
  hipError_t e = launch();
  (void)hipEventRecord(r.e1, st);
  c->prof.rec[slot].push_back(r);
  return e;
}
hipError_t prof_conv(sslcr_ctx* c, int dt, const ConvArgs& a, const ConvPlan& plan, hipStream_t st) {
  auto book = [&](ProfRec& r) {
    const double es = c->esz();
    const double rs = a.tap_mask ? (double)__builtin_popcount(a.tap_mask) : (double)a.R * a.S;
    const double M = (double)a.N * a.PH * a.PW, src = (double)a.N * a.H * a.W;
    r.flops = a.transposed ? 2.0 * src * a.C * a.K * rs : 2.0 * M * a.K * a.C * rs;
    r.bytes = (src * a.C + (double)a.K * rs * a.C + M * a.K * (a.residual ? 2.0 : 1.0) * (a.accumulate ? 2.0 : 1.0)) * es;
    r.name = plan.name;
  };
  return profiled(c, 0, st, book, [&] { return launch_conv(dt, a, plan, st); });
}
hipError_t prof_conv(sslcr_ctx* c, int dt, const ConvArgs& a, hipStream_t st) { return prof_conv(c, dt, a, conv_plan(dt, a), st); }
// a downsampling block's conv1 (3x3 / 2) and 1x1 / 2 projection of one input in one launch (conv_s2.hip)
hipError_t prof_conv_pair(sslcr_ctx* c, const ConvArgs& a, const ConvArgs& d, hipStream_t st) {
  auto book = [&](ProfRec& r) {
    const double es = c->esz();
    const double M = (double)a.N * a.PH * a.PW, src = (double)a.N * a.H * a.W;
    r.flops = 2.0 * M * a.K * a.C * 10.0;
    r.bytes = (src * a.C + (double)a.K * 10.0 * a.C + 2.0 * M * a.K) * es;
    r.name = conv_s2_name(a, true);
  };
  return profiled(c, 0, st, book, [&] { return launch_conv_s2(a, &d, st); });
}
inline bool fp8_layer(const sslcr_ctx* c, const ConvL& L) {
  return c->fp8 && L.k == 3 && L.stride == 1 && L.cin % 128 == 0 && L.cout % 128 == 0;
}
// forward conv of layer L (folded = eval pack): the fp8 kernel where the mode, the layer and the shape allow it (use_fp8), else the
// engine dtype's kernel
inline bool use_fp8(const sslcr_ctx* c, const ConvL& L, const ConvArgs& a) { return fp8_layer(c, L) && L.w8_fwd && conv_fp8_mode(a) != 0; }
hipError_t prof_conv_fp8(sslcr_ctx* c, const ConvArgs& a, const ConvL& L, bool folded, hipStream_t st) {
  Fp8Args q;
  q.w8 = folded ? L.w8_fold : L.w8_fwd;
  q.w_dequant = folded ? L.dq_fold : L.dq_fwd;
  // per-tensor activation scale by DELAYED scaling: this launch records the amax of what it quantises, the next forward of
  // this net in this mode uses 2^floor(log2(448 / (2 amax))) (scale 1 until then); no host sync anywhere
  q.x_scale = 1.0f;
  q.x_scale_dev = L.f8s ? L.f8s + (folded ? 2 : 0) : nullptr;
  q.amax_out = L.f8s ? L.f8s + (folded ? 3 : 1) : nullptr;
  auto book = [&](ProfRec& r) {
    const double M = (double)a.N * a.PH * a.PW;
    r.flops = 2.0 * M * a.K * a.C * 9.0;
    r.bytes = ((double)a.N * a.H * a.W * a.C + M * a.K * (a.residual ? 2.0 : 1.0)) * 2.0 + (double)a.K * 9.0 * a.C;
    r.name = conv_fp8_name(a);
  };
  return profiled(c, 0, st, book, [&] { return launch_conv_fp8(a, q, st); });
}
hipError_t prof_conv_fwd(sslcr_ctx* c, int dt, const ConvArgs& a_in, const ConvL& L, bool folded, hipStream_t st) {
  // (the e4m3 eval pack is the FOLDED filter with its own per-kout dequant factor: no output scale on that path)
  ConvArgs a = a_in;
  a.out_scale = nullptr;
  return use_fp8(c, L, a) ? prof_conv_fp8(c, a, L, folded, st) : prof_conv(c, dt, a_in, st);
}
hipError_t prof_wgrad(sslcr_ctx* c, int dt, const WgradArgs& a, hipStream_t st) {
  const WgradPlan plan = wgrad_plan(dt, a);
  auto book = [&](ProfRec& r) {
    const double es = c->esz();
    const double M = (double)a.N * a.OH * a.OW;
    r.flops = 2.0 * M * a.K * a.C * a.R * a.S;
    r.bytes = ((double)a.N * a.H * a.W * a.C + M * a.K) * es + (double)a.K * a.R * a.S * a.C * 4.0;
    r.name = plan.name;
  };
  return profiled(c, 1, st, book, [&] { return launch_wgrad(dt, a, plan, st); });
}

// the 16x16-tile kernels (conv3x3_h16 / conv3x3_pp64): the ones with the BatchNorm-backward front end (sslcr_conv_desc.mask_x)
inline bool tile16(const ConvPlan& p) { return p.route == ConvRoute::H16 || p.route == ConvRoute::PP64; }

constexpr int kMaxSeg = 3;      // TripletNet branches run as segments of one launch (backbone_forward)
const int kBlockCfg[8][3] ={{64, 64, 1}, {64, 64, 1}, {64, 128, 2}, {128, 128, 1}, {128, 256, 2}, {256, 256, 1}, {256, 512, 2}, {512, 512, 1}};

inline int out_dim(int h, int k, int stride, int pad) { return (h + 2 * pad - k) / stride + 1; }

void build_topology(sslcr_net* n) {
  int p = 0, nl = 0;
  n->psize.assign(n->nparams, 0);
  n->block_conv.assign(n->nparams, nullptr);
  // the next layer: parameters p (filter), p + 1, p + 2 (BatchNorm weight, bias)
  auto layer = [&](ConvL& L, BnL& bn, int cin, int cout, int k, int stride, int pad) {
    L = ConvL{cin, cout, k, stride, pad, p};
    bn = BnL{cout, p + 1, p + 2, nl};
    n->psize[p] = cout * cin * k * k;
    n->psize[p + 1] = n->psize[p + 2] = cout;
    if (nl > 0) n->block_conv[p] = &L;
    n->layers[nl++] = Layer{&L, &bn};
    p += 3;
  };
  layer(n->stem, n->bn0, 3, 64, 7, 2, 3);
  for (int i = 0; i < 8; ++i) {
    BlockL& B = n->blocks[i];
    const int cin = kBlockCfg[i][0], cout = kBlockCfg[i][1], s = kBlockCfg[i][2];
    B.pstart = p;
    layer(B.c1, B.b1, cin, cout, 3, s, 1);
    layer(B.c2, B.b2, cout, cout, 3, 1, 1);
    B.has_ds = (s != 1 || cin != cout);
    if (B.has_ds) layer(B.ds, B.bd, cin, cout, 1, s, 0);
  }
  // p == 60, nl == kLayers ; heads: 60 fc.0.weight [512,1024], 61 fc.0.bias, 62 fc.2.weight [256,512], 63 fc.2.bias, 64.. classifier
  n->psize[60] = 512 * 1024;
  n->psize[61] = 512;
  n->psize[62] = 256 * 512;
  n->psize[63] = 256;
  if (n->head_kind == 0) {
    n->psize[64] = n->ncls * 768;
    n->psize[65] = n->ncls;
  } else {
    n->psize[64] = 128 * 768;
    n->psize[65] = 128;
    n->psize[66] = n->ncls * 128;
    n->psize[67] = n->ncls;
  }
  n->goff.assign(n->nparams + 1, 0);
  for (int i = 0; i < n->nparams; ++i) n->goff[i + 1] = n->goff[i] + ((n->psize[i] + 63) & ~63);
  n->grad_count = n->goff[n->nparams];
}

// bf16 storage: eval-mode BatchNorm is NOT folded into the filters (the scale rides in the conv epilogues).  SSLCR_UNFOLD_EVAL=0 folds as
// rounds 1-5 did (A/B runs, tools/bf16_teacher_fold_experiment.py)
bool unfold_eval(const sslcr_ctx* c) { return sw::on(sw::UNFOLD_EVAL) && c->dtype == DT_BF16; }

int alloc_shadow(sslcr_net* n) {
  const size_t es = n->ctx->esz();
  Carver c;
  // where take() put each pack of each layer, in the order of the buffer (kNone: this layer has no such pack)
  constexpr size_t kNone = ~(size_t)0;
  struct Off { size_t w_fwd, w_dg, w_fold, b_fold, s_fold, w_foldf = kNone, w8_fwd = kNone, w8_fold = kNone, dq_fwd = kNone, dq_fold = kNone; };
  Off off[kLayers];
  for (int l = 0; l < kLayers; ++l) {
    const ConvL& L = *n->layers[l].conv;
    Off& o = off[l];
    const bool stem = L.pidx == 0;
    const size_t wbytes = (stem ? (size_t)64 * 224 : (size_t)L.cout * L.cin * L.k * L.k) * es, kbytes = L.cout * sizeof(float);
    o.w_fwd = c.take(wbytes);
    o.w_dg = c.take(wbytes);
    o.w_fold = c.take(wbytes);
    o.b_fold = c.take(kbytes);
    o.s_fold = c.take(kbytes);                      // (the room is there in either mode)
    if (!unfold_eval(n->ctx)) o.s_fold = kNone;
    if (stem) o.w_foldf = c.take(wbytes);
    if (fp8_layer(n->ctx, L)) {
      o.w8_fwd = c.take((size_t)L.cout * 9 * L.cin);
      o.w8_fold = c.take((size_t)L.cout * 9 * L.cin);
      o.dq_fwd = c.take(kbytes);
      o.dq_fold = c.take(kbytes);
    }
  }
  TRYI(n->shadow.ensure(c.off));
  auto at = [&](size_t o) { return o == kNone ? nullptr : (char*)n->shadow.p + o; };
  for (int l = 0; l < kLayers; ++l) {
    ConvL& L = *n->layers[l].conv;
    const Off& o = off[l];
    L.w_fwd = at(o.w_fwd); L.w_dg = at(o.w_dg); L.w_fold = at(o.w_fold); L.w_foldf = at(o.w_foldf);
    L.b_fold = (float*)at(o.b_fold); L.s_fold = (float*)at(o.s_fold);
    L.w8_fwd = (uint8_t*)at(o.w8_fwd); L.w8_fold = (uint8_t*)at(o.w8_fold);
    L.dq_fwd = (float*)at(o.dq_fwd); L.dq_fold = (float*)at(o.dq_fold);
  }
  if (n->ctx->fp8) {
    n->n8 = 0;
    for (const Layer& ly : n->layers) if (ly.conv->w8_fwd) n->n8 += 2;
    TRYI(n->f8buf.ensure((size_t)n->n8 * 2 * sizeof(float)));
    n->f8slots = (float*)n->f8buf.p;
    std::vector<float> init((size_t)n->n8 * 2);
    for (int i = 0; i < n->n8; ++i) { init[2 * i] = 1.f; init[2 * i + 1] = 0.f; }
    TRY(hipMemcpy(n->f8slots, init.data(), init.size() * sizeof(float), hipMemcpyHostToDevice));
    int k = 0;
    for (const Layer& ly : n->layers) if (ly.conv->w8_fwd) { ly.conv->f8s = n->f8slots + 4 * k; ++k; }
  }
  return 0;
}

// the e4m3 packs of a layer the fp8 kernel serves (mode bit 0: train, bit 1: eval-folded); nothing for the others
int pack_fp8_layer(sslcr_net* n, const ConvL& L, const BnL& bn, int mode, hipStream_t st) {
  if (!L.w8_fwd) return 0;
  PackFp8Args f;
  memset(&f, 0, sizeof(f));
  f.w = n->params[L.pidx]; f.K = L.cout; f.C = L.cin; f.eps = 1e-5f;
  if (mode & 1) {
    f.w8 = L.w8_fwd; f.w_dequant = L.dq_fwd;
    TRY(launch_pack_fp8(f, st));
  }
  if (mode & 2) {
    f.w8 = L.w8_fold; f.w_dequant = L.dq_fold;
    f.gamma = n->params[bn.pg]; f.beta = n->params[bn.pb]; f.rmean = n->bn_rm[bn.bidx]; f.rvar = n->bn_rv[bn.bidx];
    TRY(launch_pack_fp8(f, st));        // (the folded bias is the bf16 pack's b_fold)
  }
  return 0;
}

int pack_conv_layer(sslcr_net* n, ConvL& L, const BnL& bn, int mode, hipStream_t st) {
  const int dt = n->ctx->dtype;
  PackArgs a;
  memset(&a, 0, sizeof(a));
  a.w = n->params[L.pidx];
  a.K = L.cout; a.C = L.cin; a.R = L.k; a.S = L.k;
  a.eps = 1e-5f;
  const bool stem = (L.pidx == 0);
  if (mode & 1) {
    a.w_fwd = L.w_fwd;
    a.w_dgrad = stem ? nullptr : L.w_dg;
    a.dgrad_flip = (L.k == 3 && L.stride == 1);     // stride-1 dgrad runs as a plain 3x3 conv of dY (halo kernel)
    TRY(stem ? launch_pack_stem(dt, a, st) : launch_pack_conv(dt, a, st));
  }
  if (mode & 2) {
    a.w_fwd = L.w_fold;
    a.w_dgrad = nullptr;
    a.gamma = n->params[bn.pg]; a.beta = n->params[bn.pb];
    a.rmean = n->bn_rm[bn.bidx]; a.rvar = n->bn_rv[bn.bidx];
    a.bias_out = L.b_fold;
    a.scale_out = L.s_fold;                          // (non-null: w_fold is the plain filter, the scale goes to the epilogue)
    TRY(stem ? launch_pack_stem(dt, a, st) : launch_pack_conv(dt, a, st));
    if (stem && L.s_fold && L.w_foldf) {             // ... and the folded form for the stem's two-kernel path
      a.w_fwd = L.w_foldf; a.scale_out = nullptr;
      TRY(launch_pack_stem(dt, a, st));
    }
  }
  return pack_fp8_layer(n, L, bn, mode, st);
}

// ---------------------------------------------------------------- BN finalize (optionally synced across ranks)
// the descriptor of one BatchNorm's finalize launch, all but its count, segments and sums: what finalize_bn and finalize_bn_pair share
BnFinalizeArgs bn_finalize_args(sslcr_net* n, const BnL& bn, const float* partials, int rows, BnSaved& sv, int replay) {
  sslcr_ctx* c = n->ctx;
  BnFinalizeArgs a;
  memset(&a, 0, sizeof(a));
  a.partials = partials; a.rows = rows; a.C = bn.C;
  a.gamma = n->params[bn.pg]; a.beta = n->params[bn.pb];
  a.scale = sv.scale; a.shift = sv.shift; a.mean = sv.mean; a.invstd = sv.invstd;
  a.running_mean = n->bn_rm[bn.bidx]; a.running_var = n->bn_rv[bn.bidx]; a.num_batches_tracked = n->bn_nbt[bn.bidx];
  if (n->f8_calib_pass) { a.running_mean = nullptr; a.running_var = nullptr; a.num_batches_tracked = nullptr; }
  a.momentum = 0.1f; a.eps = 1e-5f; a.replay = replay;
  a.stage = c->bn_stage; a.tickets = c->bn_tickets;
  return a;
}

// nseg > 1: `rows` covers nseg segments (equal shares, in order), sv is segment 0's and the others follow seg_stride floats apart
int finalize_bn(sslcr_net* n, const BnL& bn, const float* partials, int rows, double local_count, BnSaved& sv, int replay, hipStream_t st,
                int nseg = 1, int seg_stride = 0) {
  sslcr_ctx* c = n->ctx;
  if (nseg > 1 && sharded(c) && c->bn_sync) return fail("finalize_bn: segments with synced BatchNorm");
  BnFinalizeArgs a = bn_finalize_args(n, bn, partials, rows, sv, replay);
  a.nseg = nseg; a.seg_stride = seg_stride;
  if (sharded(c) && c->bn_sync) {
    // global-batch statistics: reduce rows -> [2][C] sums, all-reduce, finalize from the sums
    BnFinalizeArgs r = a;
    r.sums_out = c->bn_sums;
    TRY(launch_bn_finalize(r, st));
    TRYI(all_reduce(c, 0, c->bn_sums, 2 * (size_t)bn.C, true, st));
    a.sums_in = c->bn_sums;
    a.count = local_count * c->world;
  } else {
    a.count = local_count;
  }
  TRY(launch_bn_finalize(a, st));
  return 0;
}

// a downsampling block's bn1 and projection BatchNorm, whose statistics rows come out of ONE launch (the stride-2 pair): with synced
// BatchNorm their sums share one all-reduce ([2][C] each, adjacent in bn_sums) -- 3 of the step's 37 latency-bound collectives less
int finalize_bn_pair(sslcr_net* n, const BnL& b1, const float* part1, int rows1, const BnL& bd, const float* partd, int rowsd, double local_count,
                     BnSaved& sv1, BnSaved& svd, int replay, hipStream_t st, int nseg, int seg_stride) {
  sslcr_ctx* c = n->ctx;
  if (!(sharded(c) && c->bn_sync) || b1.C != bd.C || nseg > 1) {
    TRYI(finalize_bn(n, b1, part1, rows1, local_count, sv1, replay, st, nseg, seg_stride));
    return finalize_bn(n, bd, partd, rowsd, local_count, svd, replay, st, nseg, seg_stride);
  }
  BnFinalizeArgs a[2] = {bn_finalize_args(n, b1, part1, rows1, sv1, replay), bn_finalize_args(n, bd, partd, rowsd, svd, replay)};
  for (int i = 0; i < 2; ++i) {
    BnFinalizeArgs r = a[i];
    r.sums_out = c->bn_sums + (size_t)i * 2 * b1.C;
    TRY(launch_bn_finalize(r, st));                  // rows -> this rank's sums (the stage is consumed before the next launch reuses it)
  }
  TRYI(all_reduce(c, 0, c->bn_sums, 4 * (size_t)b1.C, true, st));
  for (int i = 0; i < 2; ++i) {
    a[i].sums_in = c->bn_sums + (size_t)i * 2 * b1.C;
    a[i].count = local_count * c->world;
    TRY(launch_bn_finalize(a[i], st));
  }
  return 0;
}

ConvArgs conv_args(const ConvL& L, const void* x, const void* w, void* y, int N, int H, int W) {
  ConvArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = w; a.y = y;
  a.N = N; a.H = H; a.W = W; a.C = L.cin; a.K = L.cout; a.R = L.k; a.S = L.k; a.stride = L.stride; a.pad = L.pad;
  a.PH = out_dim(H, L.k, L.stride, L.pad); a.PW = out_dim(W, L.k, L.stride, L.pad);
  a.OH = a.PH; a.OW = a.PW; a.osh = 1;
  return a;
}

// the statistics buffer of a launch that writes nrows partial rows
int partials_rows(sslcr_ctx* c, int nrows, int K, float** out) {
  TRYI(c->partials.ensure((size_t)nrows * 2 * K * sizeof(float)));
  *out = (float*)c->partials.p;
  return 0;
}
int ensure_partials(sslcr_ctx* c, const ConvArgs& a, float** out, int* rows) {
  *rows = conv_plan(DT_BF16, a).rows;      // (asked before the dtype's launch: the routes tile alike in both)
  return partials_rows(c, *rows, a.K, out);
}

struct Dims {
  int oh0, ow0, ph, pw;
  int lh[8], lw[8];     // OUTPUT spatial dims of each block
};
Dims make_dims(int H, int W) {
  Dims d;
  d.oh0 = out_dim(H, 7, 2, 3); d.ow0 = out_dim(W, 7, 2, 3);
  d.ph = out_dim(d.oh0, 3, 2, 1); d.pw = out_dim(d.ow0, 3, 2, 1);
  int h = d.ph, w = d.pw;
  for (int i = 0; i < 8; ++i) {
    const int s = kBlockCfg[i][2];
    h = out_dim(h, 3, s, 1); w = out_dim(w, 3, s, 1);
    d.lh[i] = h; d.lw[i] = w;
  }
  return d;
}

// Saved activations of ALL passes (1, or the 3 TripletNet branches) in one buffer, laid out [tensor][pass][...]: a tensor of
// pass p+1 follows the same tensor of pass p, so a weight-gradient launch can take the branches as one 3N-image batch
// (dW is linear in the pixels; at N=128 per branch the per-launch fp32 atomics into dW dominated the RSP step).
int alloc_passes(sslcr_net* n, int npass, int N, int H, int W) {
  const size_t es = n->ctx->esz();
  const Dims d = make_dims(H, W);
  Carver c;
  auto take = [&](size_t per_pass) { return c.take(per_pass * npass); };   // (every per-pass size is a multiple of 128 bytes)
  const size_t s_raw0 = (size_t)N * d.oh0 * d.ow0 * 64 * es, s_pool = (size_t)N * d.ph * d.pw * 64 * es, s_arg = (size_t)N * d.ph * d.pw * 64;
  const size_t o_raw0 = take(s_raw0), o_pool = take(s_pool), o_arg = take(s_arg);
  size_t o_blk[8][4], s_blk[8], o_bits[8], s_bits[8];
  bool bits_ok = true;
  for (int i = 0; i < 8; ++i) {
    s_blk[i] = (size_t)N * d.lh[i] * d.lw[i] * kBlockCfg[i][1] * es;
    for (int j = 0; j < 4; ++j) o_blk[i][j] = (j == 2 && !n->blocks[i].has_ds) ? 0 : take(s_blk[i]);
    s_bits[i] = (((size_t)N * d.lh[i] * d.lw[i] * kBlockCfg[i][1] / 8) + 127) / 128 * 128;
    o_bits[i] = take(s_bits[i]);
    if (s_bits[i] * 8 != (size_t)N * d.lh[i] * d.lw[i] * kBlockCfg[i][1]) bits_ok = false;      // padded: not contiguous across passes
  }
  const size_t s_bn = 20 * 4 * 512 * sizeof(float), s_E = (size_t)N * 512 * sizeof(float);
  const size_t o_bn = take(s_bn), o_E = take(s_E);
  TRYI(n->pass[0].mem.ensure(c.off));
  char* b = (char*)n->pass[0].mem.p;
  for (int p = 0; p < npass; ++p) {
    PassState& ps = n->pass[p];
    ps.raw0 = b + o_raw0 + p * s_raw0; ps.pooled = b + o_pool + p * s_pool; ps.argmax = (uint8_t*)(b + o_arg + p * s_arg);
    for (int i = 0; i < 8; ++i) {
      ps.blk[i].raw1 = b + o_blk[i][0] + p * s_blk[i]; ps.blk[i].raw2 = b + o_blk[i][1] + p * s_blk[i];
      ps.blk[i].rawd = n->blocks[i].has_ds ? b + o_blk[i][2] + p * s_blk[i] : nullptr;
      ps.blk[i].y = b + o_blk[i][3] + p * s_blk[i];
      ps.blk[i].ybits = (uint8_t*)(b + o_bits[i] + p * s_bits[i]);
    }
    float* f = (float*)(b + o_bn + p * s_bn);
    for (int i = 0; i < 20; ++i) {
      ps.bn[i] = BnSaved{f, f + 512, f + 1024, f + 1536};
      f += 2048;
    }
    ps.E = (float*)(b + o_E + p * s_E);
    ps.N = N; ps.H = H; ps.W = W;
  }
  n->ybits_ok = bits_ok;
  return 0;
}

// ---------------------------------------------------------------- backbone forward, train mode (saves everything)
// the descriptors of the stem conv and of the max-pool behind it, like conv_args: shape and tensors; the mode's fields are the caller's
StemArgs stem_args(const void* x, const void* w, void* y, int in_f32, int N, int H, int W, const Dims& d) {
  StemArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.w = w; a.y = y;
  a.N = N; a.H = H; a.W = W; a.OH = d.oh0; a.OW = d.ow0; a.in_f32 = in_f32;
  return a;
}
PoolFwdArgs pool_args(const void* x, void* y, int N, const Dims& d) {
  PoolFwdArgs p;
  memset(&p, 0, sizeof(p));
  p.x = x; p.y = y;
  p.N = N; p.H = d.oh0; p.W = d.ow0; p.C = 64; p.OH = d.ph; p.OW = d.pw;
  return p;
}

// stem of one pass: conv1 7x7/2 with statistics -> bn0 finalize -> BatchNorm + ReLU + max-pool into ps.pooled
int forward_stem(sslcr_net* n, PassState& ps, const void* x, int in_f32, int N, int H, int W, int replay, hipStream_t st) {
  sslcr_ctx* c = n->ctx;
  const int dt = c->dtype;
  const Dims d = make_dims(H, W);
  ps.x = x; ps.in_f32 = in_f32;
  StemArgs a = stem_args(x, n->stem.w_fwd, ps.raw0, in_f32, N, H, W, d);
  a.x2 = ps.x2; a.n_split = ps.n_split;
  const int rows = stem_partials_rows(a);
  TRYI(c->partials.ensure((size_t)rows * 2 * 64 * sizeof(float)));
  a.stats = (float*)c->partials.p;
  TRY(launch_stem(dt, a, st));
  TRYI(finalize_bn(n, n->bn0, a.stats, rows, (double)N * d.oh0 * d.ow0, ps.bn[0], replay, st));
  PoolFwdArgs p = pool_args(ps.raw0, ps.pooled, N, d);
  p.scale = ps.bn[0].scale; p.shift = ps.bn[0].shift; p.argmax = ps.argmax;
  TRY(launch_bn_relu_maxpool(dt, p, st));
  return 0;
}

// The ReLU mask of a block output as bits (sslcr_bn_act_desc.ybits, bf16 mode): bn2's backward reduce pass reads 1/16 of the bytes of y.
// SSLCR_YBITS=0 keeps the tensor read (same-box A/B runs).
bool ybits_on(const sslcr_ctx* c) { return sw::on(sw::YBITS) && c->dtype == DT_BF16; }
// the bits that go with the saved output of block i (nullptr: this net keeps none)
uint8_t* ybits_of(const sslcr_net* n, const PassState& ps, int i) { return n->ybits_ok && ybits_on(n->ctx) ? ps.blk[i].ybits : nullptr; }

// THE BLOCK PLAN: everything the train-mode forward of block i decides, for `nseg` passes of N images each whose first is ps.  The only
// place that fills the block forward's conv descriptors: forward_blocks launches from it and segments_servable asks it, so the two
// cannot disagree.  What is still missing is where the statistics rows go: offsets here, pointers once ctx->partials is large enough.
struct ConvStage {
  const ConvL* L;
  ConvArgs a;
  ConvPlan plan;                // of `a` in the engine's dtype: what the launch switches on
  bool fp8;                     // the e4m3 kernel takes it instead
  int rows;                     // statistics rows the launch writes ...
  size_t stats_off;             // ... at this offset of ctx->partials
  size_t stats_bytes() const { return (size_t)rows * 2 * a.K * sizeof(float); }
};
struct BlockPlan {
  ConvStage c1, c2, ds;         // (ds: blocks with a projection shortcut)
  // a downsampling block's conv1 and projection read the same input: one launch where the plane-gather kernel serves the pair; else
  // two (fp32, layer4.0's 8x8 maps, ragged shapes)
  bool paired;
  bool seg_ok;                  // every launch has a form for these segments and its rows split evenly among them
  int seg_stride;               // floats from one pass's saved BatchNorm statistics to the next pass's
  // bytes of ctx->partials that conv1 and the projection need together; conv2 then needs its own stats_bytes().  forward_blocks grows
  // the buffer in these two steps, not once to the larger: reserving the maximum up front left every output bit alone and measured
  // 0.02 ms per step slower on the same box, twice (another hipFree / hipMalloc history: profiles/engine_forward_refactor_ab.txt)
  size_t c1_ds_bytes;
};
BlockPlan block_plan(sslcr_net* n, const PassState& ps, const Dims& d, int i, int N, int nseg) {
  sslcr_ctx* c = n->ctx;
  const int dt = c->dtype;
  const BlockL& B = n->blocks[i];
  const bool segs = nseg > 1;
  const int xh = i ? d.lh[i - 1] : d.ph, xw = i ? d.lw[i - 1] : d.pw;
  const char* X = i ? ps.blk[i - 1].y : ps.pooled;
  BlockPlan bp{};
  bp.seg_stride = segs ? (int)(n->pass[1].bn[0].scale - n->pass[0].bn[0].scale) : 0;
  // pro: the BatchNorm + ReLU the conv applies to its input on the way in
  auto stage = [&](ConvStage& s, const ConvL& L, const void* x, void* y, int h, int w, const BnSaved* pro) {
    s.L = &L;
    s.a = conv_args(L, x, L.w_fwd, y, nseg * N, h, w);
    if (pro) { s.a.in_scale = pro->scale; s.a.in_shift = pro->shift; s.a.in_relu = 1; }
    if (segs) { s.a.seg_images = N; s.a.seg_stride = pro ? bp.seg_stride : 0; }
    s.a.stats = c->zeros;         // (stands for its region of ctx->partials until forward_blocks has it: the predicates look at the mode only)
    s.fp8 = !segs && use_fp8(c, L, s.a);
    s.plan = conv_plan(dt, s.a);
    // (the rows buffer has no dtype: the routes tile alike in both)
    s.rows = s.fp8 ? conv_fp8_rows(s.a) : dt == DT_BF16 ? s.plan.rows : conv_plan(DT_BF16, s.a).rows;
  };
  stage(bp.c1, B.c1, X, ps.blk[i].raw1, xh, xw, nullptr);
  stage(bp.c2, B.c2, ps.blk[i].raw1, ps.blk[i].raw2, d.lh[i], d.lw[i], &ps.bn[B.b1.bidx]);
  bp.seg_ok = bp.c1.plan.seg_ok && bp.c2.plan.seg_ok && bp.c1.rows % nseg == 0 && bp.c2.rows % nseg == 0;
  // ctx->partials: conv1's rows, the projection's behind them; conv2 takes the buffer over from its start -- by then both finalizes
  // have consumed what was there
  Carver cv;
  bp.c1.stats_off = cv.take(bp.c1.stats_bytes());
  if (B.has_ds) {
    stage(bp.ds, B.ds, X, ps.blk[i].rawd, xh, xw, nullptr);
    bp.paired = !bp.c1.fp8 && conv_s2_pair_ok(dt, bp.c1.a, bp.ds.a);
    if (bp.paired) bp.ds.rows = bp.c1.rows;       // (the pair kernel writes both sets of rows per tile of conv1)
    bp.seg_ok = bp.seg_ok && bp.ds.plan.seg_ok && bp.ds.rows % nseg == 0;
    bp.ds.stats_off = cv.take(bp.ds.stats_bytes());
  }
  bp.c1_ds_bytes = cv.off;
  bp.c2.stats_off = 0;
  return bp;
}
hipError_t launch_stage(sslcr_ctx* c, const ConvStage& s, hipStream_t st) {
  return s.fp8 ? prof_conv_fp8(c, s.a, *s.L, false, st) : prof_conv(c, c->dtype, s.a, s.plan, st);
}

// the eight residual blocks + average pool from ps.pooled on.  nseg == 1: one pass of N images.  nseg > 1: ps is the FIRST of nseg
// passes whose saved tensors follow one another (alloc_passes) -- every layer is then one launch over nseg * N images with
// seg_images = N in its descriptor, one finalize and one bn_act for the nseg BatchNorm batches (see segments_servable)
int forward_blocks(sslcr_net* n, PassState& ps, int N, int H, int W, int replay, int nseg, hipStream_t st) {
  sslcr_ctx* c = n->ctx;
  const int dt = c->dtype;
  const Dims d = make_dims(H, W);
  for (int i = 0; i < 8; ++i) {
    BlockL& B = n->blocks[i];
    BlockPlan bp = block_plan(n, ps, d, i, N, nseg);
    if (nseg > 1 && !bp.seg_ok) return fail("forward_blocks: block %d has no segment form here (segments_servable read the same plan)", i);
    n->fwd_flags[i] = (nseg > 1 ? 1 << 6 : 0) | (bp.paired ? 1 << 7 : 0);
    // every conv with statistics is the same three steps over its region of ctx->partials: reserve, launch, finalize
    auto reserve = [&](size_t bytes, std::initializer_list<ConvStage*> stages) {
      TRYI(c->partials.ensure(bytes));
      for (ConvStage* s : stages) s->a.stats = (float*)((char*)c->partials.p + s->stats_off);
      return 0;
    };
    TRYI(reserve(bp.c1_ds_bytes, {&bp.c1, &bp.ds}));
    const double cnt = (double)N * d.lh[i] * d.lw[i];
    BnSaved &sv1 = ps.bn[B.b1.bidx], &sv2 = ps.bn[B.b2.bidx];
    // conv1, and the projection in the same launch or right behind it, so that the two BatchNorms share one all-reduce of their sums
    // when BatchNorm is synced across ranks
    if (bp.paired) {
      TRY(prof_conv_pair(c, bp.c1.a, bp.ds.a, st));
    } else {
      TRY(launch_stage(c, bp.c1, st));
      if (B.has_ds) TRY(launch_stage(c, bp.ds, st));
    }
    if (B.has_ds) {
      TRYI(finalize_bn_pair(n, B.b1, bp.c1.a.stats, bp.c1.rows, B.bd, bp.ds.a.stats, bp.ds.rows, cnt, sv1, ps.bn[B.bd.bidx], replay, st, nseg,
                            bp.seg_stride));
    } else {
      TRYI(finalize_bn(n, B.b1, bp.c1.a.stats, bp.c1.rows, cnt, sv1, replay, st, nseg, bp.seg_stride));
    }
    TRYI(reserve(bp.c2.stats_bytes(), {&bp.c2}));
    TRY(launch_stage(c, bp.c2, st));
    TRYI(finalize_bn(n, B.b2, bp.c2.a.stats, bp.c2.rows, cnt, sv2, replay, st, nseg, bp.seg_stride));
    BnActArgs e;
    memset(&e, 0, sizeof(e));
    e.x = ps.blk[i].raw2; e.scale = sv2.scale; e.shift = sv2.shift;
    e.y = ps.blk[i].y; e.pixels = (size_t)nseg * N * d.lh[i] * d.lw[i]; e.C = B.c2.cout; e.relu = 1;
    if (nseg > 1) { e.nseg = nseg; e.seg_stride = bp.seg_stride; }
    e.ybits = ybits_of(n, ps, i);
    if (B.has_ds) {
      e.res = ps.blk[i].rawd; e.rscale = ps.bn[B.bd.bidx].scale; e.rshift = ps.bn[B.bd.bidx].shift;
    } else {
      e.res = bp.c1.a.x;
    }
    TRY(launch_bn_act(dt, e, st));
  }
  TRY(launch_avgpool_fwd(dt, ps.blk[7].y, ps.E, nseg * N, d.lh[7] * d.lw[7], 512, st));
  return 0;
}

// The TripletNet branches (models/net.py:50-66: three tiles through ONE backbone, BatchNorm statistics per call) as SEGMENTS of one
// launch per layer: the saved tensors of the passes are contiguous (alloc_passes), so a conv over 3N images with
// sslcr_conv_desc.seg_images = N writes all three, its statistics rows split by segment, and one finalize / one bn_act serves the
// three BatchNorm batches (running statistics updated in branch order).  At N = 128 per branch the per-pass launches were 60 %
// slower per image than the same kernels at N = 640 (r03: conv3x3_h16 48.7 us against 149 us for five times the images).
// The stem (three separate input tensors) and its pool stay per pass.  false = some layer has no segment form here: the caller
// runs the passes one by one.
bool segments_on() { return sw::on(sw::SEGMENTS); }
// (asked once the passes are allocated for N, H, W: the plans it reads are the ones forward_blocks will launch from)
bool segments_servable(sslcr_net* n, int N, int H, int W) {
  sslcr_ctx* c = n->ctx;
  // fp8, synced BatchNorm and the profiler keep the pass-by-pass form -- which is why the fp8 calibration pass never needs the segment form
  if (!segments_on() || !n->triplet || c->dtype != DT_BF16 || c->fp8 || (sharded(c) && c->bn_sync) || c->prof.on) return false;
  const Dims d = make_dims(H, W);
  for (int i = 0; i < 8; ++i)
    if (!block_plan(n, n->pass[0], d, i, N, kMaxSeg).seg_ok) return false;
  return true;
}

// ---------------------------------------------------------------- backbone forward, eval mode (BN folded, nothing saved)
// npass > 1 (TripletNet under model.eval(): validate() of the RSP scripts): nothing in this mode depends on the batch, so the
// branches' stems write into one buffer and every block conv runs once over npass * N images
int backbone_forward_eval(sslcr_net* n, const void* const* xs, int npass, int in_f32, int N, int H, int W, float* const* E, hipStream_t st) {
  sslcr_ctx* c = n->ctx;
  const int dt = c->dtype;
  const size_t es = c->esz();
  const Dims d = make_dims(H, W);
  const int NT = npass * N;
  Carver cv;
  const size_t o_a0 = cv.take((size_t)N * d.oh0 * d.ow0 * 64 * es);
  const size_t unit1 = (size_t)N * d.ph * d.pw * 64 * es, unit = unit1 * npass;
  size_t o_buf[4];
  for (int j = 0; j < 4; ++j) o_buf[j] = cv.take(unit);
  TRYI(c->scratch.ensure(cv.off));
  char* base = (char*)c->scratch.p;
  for (int p = 0; p < npass; ++p) {
    char* pooled = base + o_buf[0] + p * unit1;
    StemArgs a = stem_args(xs[p], n->stem.w_fold, base + o_a0, in_f32, N, H, W, d);
    a.bias = n->stem.b_fold; a.relu = 1; a.out_scale = n->stem.s_fold;
    if (stem_pool_ok(dt, a, d.ph, d.pw)) {
      a.y = pooled;                                        // conv1 + folded BatchNorm + ReLU + max-pool in one launch: the conv output stays on the CU
      TRY(launch_stem_pool(dt, a, d.ph, d.pw, st));
    } else {
      if (a.out_scale) { a.w = n->stem.w_foldf; a.out_scale = nullptr; }      // (the two-kernel path takes the folded pack)
      TRY(launch_stem(dt, a, st));
      // plain max-pool: the stem's epilogue applied the folded BatchNorm + ReLU
      TRY(launch_bn_relu_maxpool(dt, pool_args(base + o_a0, pooled, N, d), st));
    }
  }
  int xi = 0, xh = d.ph, xw = d.pw;
  for (int i = 0; i < 8; ++i) {
    BlockL& B = n->blocks[i];
    char* X = base + o_buf[xi];
    char* t1 = base + o_buf[(xi + 1) & 3];
    char* td = base + o_buf[(xi + 2) & 3];
    char* Y = base + o_buf[(xi + 3) & 3];
    const int oh = d.lh[i], ow = d.lw[i];
    ConvArgs a1 = conv_args(B.c1, X, B.c1.w_fold, t1, NT, xh, xw);
    a1.bias = B.c1.b_fold; a1.relu = 1; a1.out_scale = B.c1.s_fold;
    const void* res = X;
    if (B.has_ds) {
      ConvArgs ad = conv_args(B.ds, X, B.ds.w_fold, td, NT, xh, xw);
      ad.bias = B.ds.b_fold; ad.out_scale = B.ds.s_fold;
      if (!use_fp8(c, B.c1, a1) && conv_s2_pair_ok(dt, a1, ad)) {      // conv1 and the projection in one launch
        TRY(prof_conv_pair(c, a1, ad, st));
      } else {
        TRY(prof_conv_fwd(c, dt, a1, B.c1, true, st));
        TRY(prof_conv(c, dt,ad, st));
      }
      res = td;
    } else {
      TRY(prof_conv_fwd(c, dt, a1, B.c1, true, st));
    }
    ConvArgs a2 = conv_args(B.c2, t1, B.c2.w_fold, Y, NT, oh, ow);
    a2.bias = B.c2.b_fold; a2.residual = res; a2.relu = 1; a2.out_scale = B.c2.s_fold;
    TRY(prof_conv_fwd(c, dt, a2, B.c2, true, st));
    xi = (xi + 3) & 3; xh = oh; xw = ow;
  }
  for (int p = 0; p < npass; ++p)
    TRY(launch_avgpool_fwd(dt, base + o_buf[xi] + (size_t)p * N * xh * xw * 512 * es, E[p], N, xh * xw, 512, st));
  return 0;
}

// the backbone over the net's passes in either mode; E[p] <- where pass p's embedding is.  Train mode: the TripletNet branches as
// segments where every block has the form (all stems, then each layer once), else pass by pass
int backbone_forward(sslcr_net* n, int train, const void* const* xs, int in_f32, int N, int H, int W, float** E, hipStream_t st) {
  const int npass = n->triplet ? 3 : 1;
  if (!train) {
    for (int p = 0; p < npass; ++p) E[p] = n->dE[p];         // borrow the dE buffers (unused in eval) for the embeddings
    return backbone_forward_eval(n, xs, npass, in_f32, N, H, W, E, st);
  }
  if (n->pass[0].N != N || n->pass[0].H != H || n->pass[0].W != W || !n->pass[0].mem.p) TRYI(alloc_passes(n, npass, N, H, W));
  const bool segs = segments_servable(n, N, H, W);
  const int replay = n->triplet ? 1 : 3;
  n->last_segments = segs;
  for (int p = 0; p < npass; ++p) {
    PassState& ps = n->pass[p];
    ps.x2 = n->split_x2; ps.n_split = n->split_x2 ? n->split_n : 0;      // (single-branch nets only: sslcr_step_ssl_cr)
    TRYI(forward_stem(n, ps, xs[p], in_f32, N, H, W, replay, st));
    if (!segs) TRYI(forward_blocks(n, ps, N, H, W, replay, 1, st));
    E[p] = ps.E;
  }
  return segs ? forward_blocks(n, n->pass[0], N, H, W, replay, npass, st) : 0;
}

// ---------------------------------------------------------------- heads
int alloc_heads(sslcr_net* n, int N) {
  if (n->hN >= N && n->heads.p) return 0;
  Carver c;
  size_t o_cat[3], o_h[3], o_f[3], o_dE[3];
  for (int i = 0; i < 3; ++i) {
    o_cat[i] = c.take((size_t)N * 1024 * 4); o_h[i] = c.take((size_t)N * 512 * 4);
    o_f[i] = c.take((size_t)N * 256 * 4); o_dE[i] = c.take((size_t)N * 512 * 4);
  }
  const size_t o_feats = c.take((size_t)N * 768 * 4), o_hid = c.take((size_t)N * 128 * 4), o_log = c.take((size_t)N * 64 * 4);
  const size_t o_dfeats = c.take((size_t)N * 768 * 4), o_dhid = c.take((size_t)N * 128 * 4);
  const size_t o_d256 = c.take((size_t)N * 256 * 4), o_d512 = c.take((size_t)N * 512 * 4), o_dcat = c.take((size_t)N * 1024 * 4);
  const size_t o_scr = c.take((size_t)N * 1024 * 4), o_dl = c.take((size_t)N * 64 * 4), o_lt = c.take((size_t)N * 64 * 4);
  TRYI(n->heads.ensure(c.off));
  char* b = (char*)n->heads.p;
  for (int i = 0; i < 3; ++i) {
    n->cat[i] = (float*)(b + o_cat[i]); n->hact[i] = (float*)(b + o_h[i]);
    n->fi[i] = (float*)(b + o_f[i]); n->dE[i] = (float*)(b + o_dE[i]);
  }
  n->feats = (float*)(b + o_feats); n->hid = (float*)(b + o_hid); n->logits = (float*)(b + o_log);
  n->dfeats = (float*)(b + o_dfeats); n->dhid = (float*)(b + o_dhid);
  n->dtmp256 = (float*)(b + o_d256); n->dtmp512 = (float*)(b + o_d512); n->dcat = (float*)(b + o_dcat);
  n->scratch = (float*)(b + o_scr); n->dlogits = (float*)(b + o_dl); n->logits_t = (float*)(b + o_lt);
  n->hN = N;
  return 0;
}

const int kPairs[3][2] = {{0, 1}, {1, 2}, {0, 2}};     // E12, E23, E13 (models/net.py:56-58)

// E[0..npass-1] -> feats [N,768], logits [N,C]
int heads_forward(sslcr_net* n, float* const* E, int npass, int N, hipStream_t st) {
  const float *w0 = n->params[60], *b0 = n->params[61], *w2 = n->params[62], *b2 = n->params[63];
  const int nh = (npass == 3) ? 3 : 1;
  for (int i = 0; i < nh; ++i) {
    const float* Ea = E[npass == 3 ? kPairs[i][0] : 0];
    const float* Eb = E[npass == 3 ? kPairs[i][1] : 0];
    if (Ea == Eb) {
      TRY(launch_copy2d_multi(n->cat[i], 1024, 2, 512, Ea, 512, 1, 0, N, 512, st));
    } else {
      TRY(launch_copy2d(n->cat[i], 1024, Ea, 512, N, 512, 0, st));
      TRY(launch_copy2d(n->cat[i] + 512, 1024, Eb, 512, N, 512, 0, st));
    }
    TRY(launch_linear_fwd(n->cat[i], w0, b0, n->hact[i], N, 512, 1024, 1, st));
    TRY(launch_linear_fwd(n->hact[i], w2, b2, n->fi[i], N, 256, 512, 0, st));
  }
  if (nh == 1) {
    TRY(launch_copy2d_multi(n->feats, 768, 3, 256, n->fi[0], 256, 1, 0, N, 256, st));
  } else {
    for (int i = 0; i < 3; ++i) TRY(launch_copy2d(n->feats + 256 * i, 768, n->fi[i], 256, N, 256, 0, st));
  }
  if (n->head_kind == 0) {
    TRY(launch_linear_fwd(n->feats, n->params[64], n->params[65], n->logits, N, n->ncls, 768, 0, st));
  } else {
    TRY(launch_linear_fwd(n->feats, n->params[64], n->params[65], n->hid, N, 128, 768, 1, st));
    TRY(launch_linear_fwd(n->hid, n->params[66], n->params[67], n->logits, N, n->ncls, 128, 0, st));
  }
  return 0;
}

inline float* gptr(sslcr_net* n, int pidx) { return n->rg[pidx] ? n->gw + n->goff[pidx] : nullptr; }

// dlogits -> head parameter grads and dE[0..npass-1]
int heads_backward(sslcr_net* n, const float* dlogits, int npass, int N, bool need_dE, hipStream_t st) {
  const float *w0 = n->params[60], *w2 = n->params[62];
  const bool any_fc = n->rg[60] || n->rg[61] || n->rg[62] || n->rg[63];
  if (n->head_kind == 0) {
    TRY(launch_linear_bwd(n->feats, n->params[64], dlogits, nullptr, (any_fc || need_dE) ? n->dfeats : nullptr, gptr(n, 64), gptr(n, 65),
                          N, n->ncls, 768, 0, n->scratch, st));
  } else {
    TRY(launch_linear_bwd(n->hid, n->params[66], dlogits, nullptr, n->dhid, gptr(n, 66), gptr(n, 67), N, n->ncls, 128, 0, n->scratch, st));
    TRY(launch_linear_bwd(n->feats, n->params[64], n->dhid, n->hid, (any_fc || need_dE) ? n->dfeats : nullptr, gptr(n, 64), gptr(n, 65),
                          N, 128, 768, 0, n->scratch, st));
  }
  if (!any_fc && !need_dE) return 0;
  const int nh = (npass == 3) ? 3 : 1;
  if (need_dE && nh == 3)
    for (int i = 0; i < npass; ++i) TRY(hipMemsetAsync(n->dE[i], 0, (size_t)N * 512 * 4, st));
  for (int i = 0; i < nh; ++i) {
    if (nh == 3) {
      TRY(launch_copy2d(n->dtmp256, 256, n->dfeats + 256 * i, 768, N, 256, 0, st));
    } else {   // the three identical branches of TripletNet_Finetune: gradients add (models/net.py:96-100)
      TRY(launch_copy2d_multi(n->dtmp256, 256, 1, 0, n->dfeats, 768, 3, 256, N, 256, st));
    }
    TRY(launch_linear_bwd(n->hact[i], w2, n->dtmp256, nullptr, n->dtmp512, gptr(n, 62), gptr(n, 63), N, 256, 512, 0, n->scratch, st));
    TRY(launch_linear_bwd(n->cat[i], w0, n->dtmp512, n->hact[i], need_dE ? n->dcat : nullptr, gptr(n, 60), gptr(n, 61), N, 512, 1024, 0,
                          n->scratch, st));
    if (need_dE && nh == 1) {                    // both halves of [E, E] are the one embedding: dE = left + right
      TRY(launch_copy2d_multi(n->dE[0], 512, 1, 0, n->dcat, 1024, 2, 512, N, 512, st));
    } else if (need_dE) {
      const int a = nh == 3 ? kPairs[i][0] : 0, b = nh == 3 ? kPairs[i][1] : 0;
      TRY(launch_copy2d(n->dE[a], 512, n->dcat, 1024, N, 512, 1, st));
      TRY(launch_copy2d(n->dE[b], 512, n->dcat + 512, 1024, N, 512, 1, st));
    }
  }
  return 0;
}

// ---------------------------------------------------------------- backbone backward for one saved pass
struct PoolSrc {            // gradient arriving through the stem max-pool (see sslcr_bn_bwd_desc.pool_dy)
  const void* dy; const uint8_t* argmax; int H, W, OH, OW; const void* y;
};

// One BatchNorm backward as its call site asks for it; what is not set is zero.
// nseg > 1 (sslcr_bn_bwd_desc.nseg): the tensors hold nseg passes one after the other, `pixels` is their total, the saved statistics
// are pass 0's (the others seg_stride floats apart), the sums nseg consecutive ring slots, sum_rows / n_sum_rows cover all passes
struct BnBwdReq {
  const void *dy = nullptr, *x = nullptr, *yact = nullptr;   // incoming gradient, saved conv output, saved block output (its ReLU mask)
  // ... and that mask as bits, where the forward kept them: whoever sets yact sets this with it (ybits_of), or the reduce pass reads
  // the whole of yact where it could read a sixteenth
  const uint8_t* yact_bits = nullptr;
  void *dx = nullptr, *gout = nullptr;                        // gradient of x; g = dy * (yact > 0) for whoever reads it next
  int relu_from_x = 0;                                        // the ReLU mask is (bn(x) > 0)
  size_t pixels = 0;
  double count = 0.0;                                         // this rank's elements per channel of ONE BatchNorm batch
  const PoolSrc* pool = nullptr;
  int g_in_reduce = 0;                                        // the reduce pass writes gout, the apply pass reads it instead of (dy, yact)
  // the dgrad that produced dy already left partial rows of (sum g, sum g (x - mean)) (sslcr_conv_desc.mask_x): no reduce pass
  const float* sum_rows = nullptr;
  int n_sum_rows = 0, nseg = 0, seg_stride = 0;
  bool defer = false;                                         // the caller launches the reduce pass itself (the two-BatchNorm form)
};

// nseg consecutive sums slots of this backward (nullptr if the ring cannot serve them)
double* take_sums_n(sslcr_ctx* c, int nseg) {
  if (!c->bn_ring.p || c->bn_ring_i + nseg > sslcr_ctx::kBnRing) return nullptr;
  double* p = (double*)c->bn_ring.p + (size_t)c->bn_ring_i * sslcr_ctx::kBnSlot;
  c->bn_ring_i += nseg;
  return p;
}
double* take_sums(sslcr_ctx* c) { return take_sums_n(c, 1); }      // the next slot
double* take_sums_or_fixed(sslcr_ctx* c) {      // one slot, or the context's fixed pair of slots when the ring is used up
  double* ring = take_sums(c);
  return ring ? ring : c->bn_sums;
}

// BatchNorm backward in three parts so that independent BatchNorms (a block's bn2 and its projection-shortcut BatchNorm) can
// share ONE all-reduce of their sums: begin = the reduce pass into `sums` ([2][C] doubles), sync = the all-reduce, end = the apply pass
int bn_bwd_begin(sslcr_net* n, const BnL& bn, const BnSaved& sv, const BnBwdReq& q, hipStream_t st, double* sums, BnBwdArgs* out) {
  sslcr_ctx* c = n->ctx;
  BnBwdArgs a;
  memset(&a, 0, sizeof(a));
  a.dy = q.dy; a.x = q.x; a.yact = q.yact; a.scale = sv.scale; a.shift = sv.shift; a.mean = sv.mean; a.invstd = sv.invstd;
  a.sums = sums; a.dx = q.dx; a.gout = q.gout; a.pixels = q.pixels; a.C = bn.C; a.relu_from_x = q.relu_from_x;
  if (q.nseg > 1) { a.nseg = q.nseg; a.seg_stride = q.seg_stride; a.sums_stride = sslcr_ctx::kBnSlot; }
  a.g_in_reduce = (q.g_in_reduce && q.yact && q.gout) ? 1 : 0;
  a.yact_bits = q.yact_bits;
  const bool synced = sharded(c) && c->bn_sync;
  if (n->rg[bn.pg] || n->rg[bn.pb]) {
    // dgamma/dbeta ride on the apply pass.  Synced BN: every rank holds the GLOBAL sums and the gradient all-reduce adds
    // `world` copies -> pre-divide (per-replica BN: the sums are this rank's share, the gradient all-reduce adds them up)
    a.dgamma = gptr(n, bn.pg); a.dbeta = gptr(n, bn.pb);
    a.pg_scale = synced ? 1.0f / c->world : 1.0f;
    if (!a.dgamma || !a.dbeta) { a.dgamma = nullptr; a.dbeta = nullptr; }
  }
  if (const PoolSrc* s = q.pool) { a.pool_dy = s->dy; a.pool_argmax = s->argmax; a.pH = s->H; a.pW = s->W; a.pOH = s->OH; a.pOW = s->OW; a.pool_y = s->y; }
  a.count = synced ? q.count * c->world : q.count;
  if (q.sum_rows) {                                 // rows -> sums
    BnFinalizeArgs r;
    memset(&r, 0, sizeof(r));
    r.partials = q.sum_rows; r.rows = q.n_sum_rows; r.C = bn.C; r.stage = c->bn_stage; r.sums_out = sums; r.tickets = c->bn_tickets;
    if (q.nseg > 1) { r.nseg = q.nseg; r.seg_stride = sslcr_ctx::kBnSlot; }
    TRY(launch_bn_finalize(r, st));
  } else if (!q.defer) {
    TRY(launch_bn_bwd_reduce(c->dtype, a, st));     // (the reduce pass overwrites its sums: nothing to clear)
  }
  *out = a;
  return 0;
}

int bn_bwd_sync(sslcr_ctx* c, double* sums, size_t count, hipStream_t st) {
  if (sharded(c) && c->bn_sync) TRYI(all_reduce(c, 0, sums, count, true, st));
  return 0;
}

int bn_bwd_end(sslcr_ctx* c, const BnBwdArgs& a, hipStream_t st) {
  auto book = [&](ProfRec& r) {
    const bool pool = a.pool_dy != nullptr;
    if (pool) r.name = c->dtype == DT_BF16 ? "sslcr::bn_bwd_apply_pool_kernel<unsigned short>" : "sslcr::bn_bwd_apply_pool_kernel<float>";
    else r.name = c->dtype == DT_BF16 ? "sslcr::bn_bwd_apply_kernel<unsigned short>" : "sslcr::bn_bwd_apply_kernel<float>";
    r.flops = 0.0;
    // algorithmic bytes: read dy (or the 4x smaller pooled gradient + 1-byte argmax), x, (saved output for the ReLU mask); write dx (, g)
    const double t = (double)a.pixels * a.C * c->esz();
    const double rd = (pool ? 0.25 * t + 0.25 * (double)a.pixels * a.C : t) + t + ((a.yact && !a.g_in_reduce) ? t : 0.0);
    r.bytes = rd + t + ((a.gout && !a.g_in_reduce) ? t : 0.0);
  };
  return check(profiled(c, 2, st, book, [&] { return launch_bn_bwd_apply(c->dtype, a, st); }), "launch_bn_bwd_apply");
}

int bn_backward(sslcr_net* n, const BnL& bn, const BnSaved& sv, const BnBwdReq& q, hipStream_t st) {
  sslcr_ctx* c = n->ctx;
  const bool segs = q.nseg > 1;                  // the passes as segments: nseg consecutive ring slots (the caller checked there are)
  double* sums = segs ? take_sums_n(c, q.nseg) : q.sum_rows ? c->bn_sums : take_sums_or_fixed(c);
  if (!sums) return fail("bn_backward: no ring slots for the segments");
  BnBwdArgs a;
  TRYI(bn_bwd_begin(n, bn, sv, q, st, sums, &a));
  if (!segs) TRYI(bn_bwd_sync(c, sums, 2 * (size_t)bn.C, st));      // (segments are not run with synced BatchNorm)
  return bn_bwd_end(c, a, st);
}

// the next writer of scratch buffer `kind` waits for the side-stream weight gradient that reads it
int wg_wait(sslcr_ctx* c, int kind, hipStream_t st) {
  if (c->wg_pending[kind]) {
    TRY(hipStreamWaitEvent(st, c->ev_wg_done[kind], 0));
    c->wg_pending[kind] = false;
  }
  return 0;
}
// `waiter` (the compute stream before the optimizer, the collective stream before a bucket) waits for every side-stream wgrad so far
int wg_join(sslcr_ctx* c, hipStream_t waiter) {
  if (!c->wg_any) return 0;
  TRY(hipEventRecord(c->ev_wg_join, c->wg_stream));
  TRY(hipStreamWaitEvent(waiter, c->ev_wg_join, 0));
  return 0;
}

// seg_images > 0: the N images are N / seg_images segments (TripletNet branches) whose producer BatchNorms sit seg_stride floats apart
// kind: which scratch buffer holds dy (0 conv2 / dRaw2, 1 conv1 / dRaw1, 2 projection / dRawD); < 0 = always on the compute stream
int wgrad_call(sslcr_net* n, const ConvL& L, const void* x, const void* dy, const BnSaved* pro, int N, int H, int W, int OH, int OW, hipStream_t st,
               int kind, int seg_images = 0, int seg_stride = 0) {
  if (!n->rg[L.pidx]) return 0;
  sslcr_ctx* c = n->ctx;
  WgradArgs a;
  memset(&a, 0, sizeof(a));
  a.x = x; a.dy = dy; a.dw = n->gw + n->goff[L.pidx];
  if (pro) { a.in_scale = pro->scale; a.in_shift = pro->shift; a.in_relu = 1; }
  a.N = N; a.H = H; a.W = W; a.C = L.cin; a.K = L.cout; a.R = L.k; a.S = L.k; a.stride = L.stride; a.pad = L.pad; a.OH = OH; a.OW = OW;
  a.seg_images = seg_images; a.seg_stride = seg_stride;
  if (kind < 0 || !c->use_wg || c->prof.on) {
    TRY(prof_wgrad(c, c->dtype, a, st));
    return 0;
  }
  if (!c->wg_stream) {
    TRY(hipStreamCreateWithFlags(&c->wg_stream, hipStreamNonBlocking));
    for (int k = 0; k < 3; ++k) {
      TRY(hipEventCreateWithFlags(&c->ev_wg_in[k], hipEventDisableTiming));
      TRY(hipEventCreateWithFlags(&c->ev_wg_done[k], hipEventDisableTiming));
    }
    TRY(hipEventCreateWithFlags(&c->ev_wg_join, hipEventDisableTiming));
  }
  TRY(hipEventRecord(c->ev_wg_in[kind], st));                  // dy (and, on the first launch, the zeroed gradient buffer) is ready
  TRY(hipStreamWaitEvent(c->wg_stream, c->ev_wg_in[kind], 0));
  TRY(prof_wgrad(c, c->dtype, a, c->wg_stream));
  TRY(hipEventRecord(c->ev_wg_done[kind], c->wg_stream));
  c->wg_pending[kind] = true;
  c->wg_any = true;
  return 0;
}

int launch_bucket_allreduce(sslcr_net* n, int bucket, size_t lo, size_t hi, hipStream_t st) {
  sslcr_ctx* c = n->ctx;
  if (!sharded(c) || hi <= lo) return 0;
  TRY(hipEventRecord(c->ev_ready[bucket], st));
  TRY(hipStreamWaitEvent(c->comm_stream, c->ev_ready[bucket], 0));
  TRYI(wg_join(c, c->comm_stream));                             // ... and the weight gradients of this bucket launched on the side stream
  float* g = n->gw + lo;
  TRYI(all_reduce(c, 1, g, hi - lo, false, c->comm_stream));
  return 0;
}

// lowest parameter index that requires grad in the backbone (60 if none)
int lowest_trainable(const sslcr_net* n) {
  for (int i = 0; i < 60; ++i)
    if (n->rg[i]) return i;
  return 60;
}

// ---------------------------------------------------------------- backbone backward, all passes
// dgrad of a 3x3 stride-1 conv: a plain conv of dy [., K] with the flipped pack [C][R][S][K]
ConvArgs dgrad3x3_s1_args(const ConvL& L, const void* dy, void* dx, int N, int oh, int ow) {
  ConvArgs a = conv_args(L, dy, L.w_dg, dx, N, oh, ow);
  a.C = L.cout; a.K = L.cin; a.transposed = 0; a.PH = oh; a.PW = ow; a.OH = oh; a.OW = ow;
  return a;
}
// ... with the BatchNorm-backward front end: the dgrad applies the ReLU mask of the BatchNorm `s` over the saved `raw` to what it
// writes and leaves that BatchNorm's two backward sums in its stats rows
ConvArgs with_bn1_mask(ConvArgs a, const void* raw, const BnSaved& s) {
  a.mask_x = raw; a.mask_scale = s.scale; a.mask_shift = s.shift; a.mask_mean = s.mean;
  return a;
}
// stride-2 3x3 dgrad: the taps an input-pixel parity class (ph % 2, pw % 2) sees -- those with (p + pad - r) even -- as bits r * 3 + s
unsigned parity_tap_mask(int ph, int pw) {
  unsigned m = 0;
  for (int r = 0; r < 3; ++r)
    for (int s = 0; s < 3; ++s)
      if (((ph + 1 - r) & 1) == 0 && ((pw + 1 - s) & 1) == 0) m |= 1u << (r * 3 + s);
  return m;
}

// One backward, walked LAYER-major: per block the BatchNorm backward / dgrad chain runs pass by pass (the reference's BatchNorm
// statistics are per branch) or, where a kernel takes the branches as segments, once; the weight gradients of conv1 and of the
// projection run ONCE over the branches' contiguous (x, dy) tensors (alloc_passes; scratch buffers of one kind are contiguous
// across passes too).  Each stage is one part of a block's backward; block() fixes their order.
// Transient buffers: one layer1-sized unit each, laid out [kind][pass], dOut and dXin being kinds 0 and 5 in turns (kOut, kXin);
// behind them one stem-sized region for dRaw0 (used pass by pass)
enum { kG = 1, kRaw2 = 2, kAct1 = 3, kRaw1 = 4, kRawD = 6, kKinds = 7 };
struct Backward {
  sslcr_net* n; sslcr_ctx* c; hipStream_t st;
  int dt, npass, N; size_t es; PassState* P; Dims d;
  int bn_stride;            // floats from one BatchNorm's saved statistics of pass p to those of pass p + 1 (the same for every BatchNorm)
  char* S; size_t unit;     // scratch base, bytes of one unit
  int kOut = 0, kXin = 5;
  // the current block (enter): geometry, and which stages take the passes as one launch
  int i; const BlockL* B;
  int oh, ow, xh, xw;       // output / input spatial dims
  size_t opix, so, si;      // per pass: output pixels, bytes of the block's output / input
  bool c2_batched, seg_dg, seg_bn;

  // pass p of a kind sits p * (tensor bytes of the current layer) behind pass 0: contiguous for the batched weight gradients
  char* buf(int kind, int p, size_t bytes) const { return S + (size_t)kind * npass * unit + (size_t)p * bytes; }
  char* dRaw0() const { return S + (size_t)kKinds * npass * unit; }
  // debug tap: slot 0 G, 1 dRaw2, 2 dAct1, 3 dRaw1, 4 dRawD, 5 dXin, 6 dOut.  src is the tensor of pass p; np > 1: of passes p .. p + np - 1,
  // one behind the other (a launch that took them as segments)
  int tap(int slot, int p, int np, const void* src, int h_, int w_, int c_) {
    if (!n->tap) return 0;
    const size_t bytes = (size_t)N * h_ * w_ * c_ * es;
    for (int j = 0; j < np; ++j) {
      DevBuf& b = n->tapbuf[p + j][i][slot];
      TRYI(b.ensure(bytes));
      TRY(hipMemcpyAsync(b.p, (const char*)src + (size_t)j * bytes, bytes, hipMemcpyDeviceToDevice, st));
      int* d4 = n->tapdims[p + j][i][slot];
      d4[0] = N; d4[1] = h_; d4[2] = w_; d4[3] = c_;
    }
    return 0;
  }

  // conv2's masked dgrad over all passes as segments: segment s masks with its own bn1
  ConvArgs conv2_dgrad_segments_args(const void* dy, void* dx) const {
    ConvArgs m = with_bn1_mask(dgrad3x3_s1_args(B->c2, dy, dx, N * npass, oh, ow), P[0].blk[i].raw1, P[0].bn[B->b1.bidx]);
    m.seg_images = N; m.seg_stride = bn_stride;
    return m;
  }

  void enter(int blk) {
    i = blk; B = &n->blocks[i];
    oh = d.lh[i]; ow = d.lw[i];
    xh = i == 0 ? d.ph : d.lh[i - 1]; xw = i == 0 ? d.pw : d.lw[i - 1];
    opix = (size_t)N * oh * ow;
    so = opix * B->c2.cout * es; si = (size_t)N * xh * xw * B->c1.cin * es;
    // conv2's weight gradient applies bn1 + ReLU of its pass to the input on the fly: the halo kernel takes the passes as
    // segments with their own (scale, shift); other shapes go pass by pass
    c2_batched = false;
    if (npass > 1) {
      WgradArgs q;
      memset(&q, 0, sizeof(q));
      q.N = N * npass; q.H = oh; q.W = ow; q.C = B->c2.cin; q.K = B->c2.cout; q.R = 3; q.S = 3; q.stride = 1; q.pad = 1; q.OH = oh; q.OW = ow;
      c2_batched = wgrad_halo_tw(q) != 0 && (wgrad_halo_tw(q) == 16 || N % 2 == 0);
    }
    // ... and conv2's dgrad with the BatchNorm-backward front end takes them as segments where the 16x16-tile kernel serves it
    seg_dg = false;
    if (npass > 1 && segments_on() && !c->prof.on) {
      const ConvArgs m = conv2_dgrad_segments_args(nullptr, nullptr);
      const ConvPlan p = conv_plan(dt, m);
      seg_dg = tile16(p) && p.seg_ok && p.rows % npass == 0;
    }
    // the elementwise BatchNorm-backward passes of the branches as segments of one launch (sslcr_bn_bwd_desc.nseg): the passes'
    // saved tensors and scratch tensors are contiguous, their saved statistics bn_stride floats apart, their sums in
    // consecutive ring slots.  Not with synced BatchNorm (one all-reduce per pass) and not under the profiler.
    seg_bn = npass > 1 && segments_on() && !c->prof.on && !(sharded(c) && c->bn_sync) && c->bn_ring.p &&
             c->bn_ring_i + 2 * npass <= sslcr_ctx::kBnRing;
    n->tap_flags[i] = (seg_bn ? 1 << 1 : 0) | (seg_dg ? 1 << 2 : 0) | (c2_batched ? 1 << 3 : 0);
  }

  // ---- bn2 stage: leaves G = dOut * (y > 0), dRaw2 and (projection shortcut) dRawD; taps 0, 1 and 4.
  // bn2's REDUCE pass forms G from the block output's ReLU mask and writes it; its apply pass, the projection shortcut's BatchNorm
  // and the identity path all read G, not (dOut, y) again.  nseg == 1: pass p; nseg == npass: all passes as segments of one launch
  int bn2(int p, int nseg) {
    const PassState& ps = P[p];
    char *G = buf(kG, p, so), *dRaw2 = buf(kRaw2, p, so), *dRawD = buf(kRawD, p, so);
    // (the previous block's side-stream weight gradients may still be reading dRaw2 / dRawD: order these writers behind them)
    TRYI(wg_wait(c, 0, st));
    if (B->has_ds) TRYI(wg_wait(c, 2, st));
    BnBwdReq q2, qd;
    q2.dy = buf(kOut, p, so); q2.x = ps.blk[i].raw2; q2.yact = ps.blk[i].y; q2.yact_bits = ybits_of(n, ps, i);
    q2.dx = dRaw2; q2.gout = G; q2.g_in_reduce = 1;
    qd.dy = G; qd.x = ps.blk[i].rawd; qd.dx = dRawD;
    q2.pixels = qd.pixels = opix * nseg; q2.count = qd.count = (double)opix;
    if (nseg > 1) { q2.nseg = qd.nseg = nseg; q2.seg_stride = qd.seg_stride = bn_stride; }
    TRYI(tap(6, p, nseg, q2.dy, oh, ow, B->c2.cout));
    if (!B->has_ds) TRYI(bn_backward(n, B->b2, ps.bn[B->b2.bidx], q2, st));
    else TRYI(nseg > 1 ? bn2_and_shortcut_segments(q2, qd) : bn2_and_shortcut(ps, q2, qd));
    TRYI(tap(0, p, nseg, G, oh, ow, B->c2.cout));
    TRYI(tap(1, p, nseg, dRaw2, oh, ow, B->c2.cout));
    return B->has_ds ? tap(4, p, nseg, dRawD, oh, ow, B->ds.cout) : 0;
  }
  int bn2_and_shortcut_segments(const BnBwdReq& q2, const BnBwdReq& qd) {
    BnBwdArgs a2, ad;
    double* sums_2 = take_sums_n(c, npass);
    if (!sums_2) return fail("backbone_backward: ring slots");
    TRYI(bn_bwd_begin(n, B->b2, P[0].bn[B->b2.bidx], q2, st, sums_2, &a2));
    TRYI(bn_bwd_begin(n, B->bd, P[0].bn[B->bd.bidx], qd, st, sums_2 + 2 * B->b2.C, &ad));
    TRYI(bn_bwd_end(c, a2, st));
    return bn_bwd_end(c, ad, st);
  }
  // one pass: the two reduce passes run back to back, so that sharded runs exchange both BatchNorms' sums ([2][C] each, adjacent
  // in one slot) in ONE all-reduce before the two apply passes
  int bn2_and_shortcut(const PassState& ps, BnBwdReq q2, BnBwdReq qd) {
    BnBwdArgs a2, ad;
    double* sums_2 = take_sums_or_fixed(c);
    q2.defer = qd.defer = true;
    TRYI(bn_bwd_begin(n, B->b2, ps.bn[B->b2.bidx], q2, st, sums_2, &a2));
    TRYI(bn_bwd_begin(n, B->bd, ps.bn[B->bd.bidx], qd, st, sums_2 + 2 * B->b2.C, &ad));
    // both BatchNorms receive the same g = dOut * (y > 0): one reduce pass forms it, writes it once and leaves both pairs of
    // sums, one apply pass reads it once for both (bn_bwd_reduce_pair_kernel); where that form does not apply, two passes each
    const bool pair = bn_bwd_pair_ok(a2, ad);
    // (g is read by nobody else in a downsampling block, so with the mask as bits it need not be written at all -- measured
    //  SLOWER, 15.81 -> 15.90 ms same box: forming g from (dOut, bits) a second time costs the apply pass more than reading it.
    //  SSLCR_BN_PAIR_G=0 selects that form; the debug tap always keeps g)
    const int keep_g = (n->tap || !a2.yact_bits || sw::on(sw::BN_PAIR_G)) ? 1 : 0;
    if (pair) n->tap_flags[i] |= 1 << 4;
    if (pair) {
      TRY(launch_bn_bwd_reduce_pair(dt, a2, ad, keep_g, st));
    } else {
      TRY(launch_bn_bwd_reduce(dt, a2, st));
      TRY(launch_bn_bwd_reduce(dt, ad, st));
    }
    TRYI(bn_bwd_sync(c, sums_2, 4 * (size_t)B->b2.C, st));
    if (!pair) {
      TRYI(bn_bwd_end(c, a2, st));
      return bn_bwd_end(c, ad, st);
    }
    auto book = [&](ProfRec& r) {
      r.name = dt == DT_BF16 ? "sslcr::bn_bwd_apply_pair_kernel<unsigned short>" : "sslcr::bn_bwd_apply_pair_kernel<float>";
      r.flops = 0.0;
      r.bytes = (keep_g ? 5.0 : 5.0625) * (double)opix * B->b2.C * c->esz();   // reads g (or dy + mask bits), x of both BatchNorms; writes both dx
    };
    return check(profiled(c, 2, st, book, [&] { return launch_bn_bwd_apply_pair(dt, a2, ad, keep_g, st); }), "launch_bn_bwd_apply_pair");
  }

  // ---- conv2 dgrad + bn1 stage: leaves dAct1 and dRaw1, tap_flags; taps 2 and 3.
  // bn1 of pass p (nseg == npass: of all passes as segments).  rows: the dgrad that wrote dAct1 applied bn1's ReLU mask and left
  // bn1's sums in its stats rows, so no reduce pass over (dAct1, raw1) is run; nullptr: bn1 masks and reduces itself
  int bn1(int p, int nseg, const float* rows, int nrows) {
    TRYI(wg_wait(c, 1, st));
    BnBwdReq q;
    q.dy = buf(kAct1, p, so); q.x = P[p].blk[i].raw1; q.relu_from_x = rows ? 0 : 1; q.dx = buf(kRaw1, p, so);
    q.pixels = opix * nseg; q.count = (double)opix; q.sum_rows = rows; q.n_sum_rows = nrows;
    if (nseg > 1) { q.nseg = nseg; q.seg_stride = bn_stride; }
    TRYI(bn_backward(n, B->b1, P[p].bn[B->b1.bidx], q, st));
    return tap(3, p, nseg, q.dx, oh, ow, B->c1.cout);
  }
  // pass p: where the 16x16-tile kernel serves this dgrad it takes the mask front end
  int conv2_dgrad_bn1(int p) {
    ConvArgs a = dgrad3x3_s1_args(B->c2, buf(kRaw2, p, so), buf(kAct1, p, so), N, oh, ow);
    const ConvArgs m = with_bn1_mask(a, P[p].blk[i].raw1, P[p].bn[B->b1.bidx]);
    float* rows = nullptr; int nrows = 0;
    const ConvPlan pm = conv_plan(dt, m);
    if (tile16(pm)) {
      nrows = pm.rows;
      TRYI(partials_rows(c, nrows, m.K, &rows));
      a = m;
      a.stats = rows;
    }
    TRY(prof_conv(c, dt, a, st));
    TRYI(tap(2, p, 1, a.y, oh, ow, B->c2.cin));
    if (rows) n->tap_flags[i] |= 1;
    return bn1(p, 1, rows, nrows);
  }
  // all passes as segments of one launch (their scratch tensors are contiguous): segment s leaves its own rows of bn1's backward
  // sums; bn1 then as segments too, or pass by pass on its share of the rows
  int conv2_dgrad_bn1_segments() {
    ConvArgs m = conv2_dgrad_segments_args(buf(kRaw2, 0, so), buf(kAct1, 0, so));
    float* rows = nullptr; int nrows = 0;
    TRYI(ensure_partials(c, m, &rows, &nrows));
    m.stats = rows;
    TRY(prof_conv(c, dt, m, st));
    TRYI(tap(2, 0, npass, m.y, oh, ow, B->c2.cin));
    n->tap_flags[i] |= 1;
    if (seg_bn) return bn1(0, npass, rows, nrows);
    const int per = nrows / npass;
    for (int p = 0; p < npass; ++p) TRYI(bn1(p, 1, rows + (size_t)p * per * 2 * B->b1.C, per));
    return 0;
  }

  // ---- weight-gradient stage (the argument of wgrad_call behind the stream: which scratch buffer the launch reads, see
  // sslcr_ctx::wg_stream): conv2 of pass p where the batched form does not take the shape; then one launch each over the npass * N
  // images (x and dy contiguous across passes) for conv2 where it is batched, conv1 and the projection
  int conv2_wgrad(int p) { return wgrad_call(n, B->c2, P[p].blk[i].raw1, buf(kRaw2, p, so), &P[p].bn[B->b1.bidx], N, oh, ow, oh, ow, st, 0); }
  int wgrads() {
    if (c2_batched)
      TRYI(wgrad_call(n, B->c2, P[0].blk[i].raw1, buf(kRaw2, 0, so), &P[0].bn[B->b1.bidx], N * npass, oh, ow, oh, ow, st, 0, N, bn_stride));
    const char* X0 = i == 0 ? P[0].pooled : P[0].blk[i - 1].y;
    TRYI(wgrad_call(n, B->c1, X0, buf(kRaw1, 0, so), nullptr, N * npass, xh, xw, oh, ow, st, 1));
    if (B->has_ds) TRYI(wgrad_call(n, B->ds, X0, buf(kRawD, 0, so), nullptr, N * npass, xh, xw, oh, ow, st, 2));
    return 0;
  }

  // ---- input-gradient stage: dXin = conv1's dgrad of dRaw1 + (identity shortcut) G or (projection) its dgrad of dRawD; tap 5.
  // Neither dgrad has a BatchNorm in it and both are independent per image: one launch over all passes
  int input_grad() {
    const int NB = N * npass;
    char* dXin = buf(kXin, 0, si);
    ConvArgs a = conv_args(B->c1, buf(kRaw1, 0, so), B->c1.w_dg, dXin, NB, oh, ow);
    a.C = B->c1.cout; a.K = B->c1.cin; a.transposed = (B->c1.stride == 1) ? 0 : 1; a.PH = xh; a.PW = xw; a.OH = xh; a.OW = xw;
    if (!B->has_ds) a.residual = buf(kG, 0, so);
    if (B->c1.stride == 1) {
      TRY(prof_conv(c, dt, a, st));
    } else {
      // stride 2: each parity class only sees 1 + 2 + 2 + 4 = 9 taps instead of 36 tap visits with three quarters zero-gathered;
      // one launch with the class on grid z where the DMA-gather kernel serves the shape, else four launches
      ConvArgs q4 = a;
      q4.pix_mul = 2; q4.PH = xh / 2; q4.PW = xw / 2; q4.par4 = 1;
      const bool one = xh % 2 == 0 && xw % 2 == 0 && conv_plan(dt, q4).par4_one_launch;
      if (one) n->tap_flags[i] |= 1 << 5;
      if (one) TRY(prof_conv(c, dt, q4, st));
      for (int par = 0; par < (one ? 0 : 4); ++par) {
        ConvArgs q = a;
        const int ph = par >> 1, pw = par & 1;
        q.pix_mul = 2; q.pix_off_h = ph; q.pix_off_w = pw;
        q.PH = (xh - ph + 1) / 2; q.PW = (xw - pw + 1) / 2;
        if (q.PH <= 0 || q.PW <= 0) continue;
        q.tap_mask = parity_tap_mask(ph, pw);
        TRY(prof_conv(c, dt, q, st));
      }
    }
    if (B->has_ds) {       // 1x1/2 projection: scatter-accumulate into the even positions of dXin
      ConvArgs s = conv_args(B->ds, buf(kRawD, 0, so), B->ds.w_dg, dXin, NB, oh, ow);
      s.C = B->ds.cout; s.K = B->ds.cin; s.stride = 1; s.pad = 0; s.PH = oh; s.PW = ow; s.OH = xh; s.OW = xw; s.osh = B->ds.stride;
      s.accumulate = 1;
      TRY(prof_conv(c, dt, s, st));
    }
    return tap(5, 0, npass, dXin, xh, xw, B->c1.cin);
  }

  // the current block from dOut down to dRaw1 / dRawD, and its weight gradients.  Where stages go pass by pass, pass p's bn2, conv2
  // weight gradient, dgrad and bn1 run before pass p + 1's
  int block() {
    if (seg_bn) TRYI(bn2(0, npass));
    for (int p = 0; p < npass; ++p) {
      if (!seg_bn) TRYI(bn2(p, 1));
      if (!c2_batched) TRYI(conv2_wgrad(p));
      if (!seg_dg) TRYI(conv2_dgrad_bn1(p));
    }
    if (seg_dg) TRYI(conv2_dgrad_bn1_segments());
    return wgrads();
  }

  // ---- stem stage, pass p: max-pool + ReLU backward -> bn0 backward -> conv1 wgrad (no dgrad: the input is data).
  // dOut (= dP, the pooled gradient) of pass p sits in its scratch unit, dRaw0 in the stem-sized region behind the units.  The
  // max-pool + ReLU backward is folded into both BatchNorm-backward passes (the un-pooled gradient is never written out).
  int stem(int p) {
    const PassState& ps = P[p];
    const PoolSrc pool{buf(kOut, p, (size_t)N * d.ph * d.pw * 64 * es), ps.argmax, d.oh0, d.ow0, d.ph, d.pw, ps.pooled};
    const size_t spix = (size_t)N * d.oh0 * d.ow0;
    BnBwdReq q;
    q.x = ps.raw0; q.relu_from_x = 1; q.pixels = spix; q.count = (double)spix; q.pool = &pool;
    StemWgradArgs w;
    memset(&w, 0, sizeof(w));
    w.x = ps.x; w.x2 = ps.x2; w.n_split = ps.n_split; w.dy = dRaw0(); w.dw = n->gw + n->goff[0];
    w.N = N; w.H = ps.H; w.W = ps.W; w.OH = d.oh0; w.OW = d.ow0; w.in_f32 = ps.in_f32;
    if (!(n->rg[0] && c->fuse_stem_bwd)) {          // two kernels: the apply pass writes dRaw0, the weight gradient reads it
      q.dx = dRaw0();
      TRYI(bn_backward(n, n->bn0, ps.bn[0], q, st));
      if (n->rg[0]) TRY(launch_stem_wgrad(dt, w, st));
      return 0;
    }
    // conv1 wgrad derives its dY tiles from the pooled gradient itself: the apply pass and its 2 x (N x 128 x 128 x 64)
    // round trip through HBM are gone (sslcr_stem_wgrad_pool)
    BnBwdArgs a;
    double* sums0 = take_sums_or_fixed(c);
    TRYI(bn_bwd_begin(n, n->bn0, ps.bn[0], q, st, sums0, &a));
    TRYI(bn_bwd_sync(c, sums0, 2 * 64, st));
    w.dy = nullptr;
    auto book = [&](ProfRec& r) {
      r.name = dt == DT_BF16 ? "sslcr::stem_wgrad_kernel<unsigned short, pool>" : "sslcr::stem_wgrad_kernel<float, pool>";
      r.flops = 0.0;        // listed with the HBM-bound kernels (0.1 flop per byte)
      const double t = (double)spix * 64 * c->esz();
      r.bytes = 0.25 * t + 0.25 * (double)spix * 64 + t + (double)N * 3 * ps.H * ps.W * (ps.in_f32 ? 4 : 1);
    };
    return check(profiled(c, 2, st, book, [&] { return launch_stem_wgrad_pool(dt, w, a, st); }), "launch_stem_wgrad_pool");
  }
};

int backbone_backward(sslcr_net* n, int npass, hipStream_t st) {
  sslcr_ctx* c = n->ctx;
  const int low = lowest_trainable(n);
  if (low >= 60) return 0;
  Backward b;
  b.n = n; b.c = c; b.st = st; b.dt = c->dtype; b.es = c->esz();
  b.P = n->pass; b.npass = npass; b.N = n->pass[0].N;
  b.d = make_dims(n->pass[0].H, n->pass[0].W);
  b.bn_stride = npass > 1 ? (int)(n->pass[1].bn[0].scale - n->pass[0].bn[0].scale) : 0;
  const Dims& d = b.d; const int N = b.N;
  b.unit = (((size_t)N * d.ph * d.pw * 64 * b.es) + 255) & ~(size_t)255;
  const size_t stem_sz = (((size_t)N * d.oh0 * d.ow0 * 64 * b.es) + 255) & ~(size_t)255;
  TRYI(c->scratch.ensure(kKinds * npass * b.unit + stem_sz));
  b.S = (char*)c->scratch.p;
  size_t hi_pending = n->goff[60];
  int bucket = 1;
  for (int p = 0; p < npass; ++p)
    TRY(launch_avgpool_bwd(b.dt, n->dE[p], b.buf(b.kOut, p, (size_t)N * d.lh[7] * d.lw[7] * 512 * b.es), N, d.lh[7] * d.lw[7], 512, st));
  for (int i = 7; i >= 0; --i) {
    b.enter(i);
    TRYI(b.block());
    const bool need_dx = low < b.B->pstart;          // something upstream of this block is trainable
    if (need_dx) {
      TRYI(b.input_grad());
      const int t = b.kOut; b.kOut = b.kXin; b.kXin = t;      // this block's input gradient is the next dOut
    }
    if (i == 6 || i == 4 || i == 2) {   // layer4 / layer3 / layer2 gradients are final: reduce them under the rest of backward
      TRYI(launch_bucket_allreduce(n, bucket++, n->goff[b.B->pstart], hi_pending, st));
      hi_pending = n->goff[b.B->pstart];
    }
    if (!need_dx) break;
  }
  if (low < 3)
    for (int p = 0; p < npass; ++p) TRYI(b.stem(p));
  TRYI(launch_bucket_allreduce(n, bucket, 0, hi_pending, st));
  return 0;
}

int net_forward(sslcr_net* n, int train, const void* const* xs, int in_f32, int N, int H, int W, float* feats, float* logits, hipStream_t st) {
  if (!(train ? n->packed_train : n->packed_eval)) TRYI(sslcr_net_pack(n, train ? 1 : 2, st));   // shadow weights are stale
  const int npass = n->triplet ? 3 : 1;
  float* E[3] = {nullptr, nullptr, nullptr};
  if (n->n8 > 0 && !n->f8_cal[train ? 0 : 1]) {
    // fp8 delayed scaling needs one forward to have seen the data: the FIRST forward of a net in a mode runs twice -- a
    // calibration pass at scale 1 (amax recorded, BatchNorm running statistics untouched, outputs overwritten below), then the
    // real one with the scales it produced
    n->f8_calib_pass = true;
    TRYI(alloc_heads(n, N));
    const int rc = backbone_forward(n, train, xs, in_f32, N, H, W, E, st);
    n->f8_calib_pass = false;
    if (rc) return rc;                           // not calibrated: the next forward tries again instead of running at scale 1
    n->f8_cal[train ? 0 : 1] = true;
  }
  if (n->n8 > 0) TRY(launch_fp8_scale_update(n->f8slots, n->n8, st));      // fp8 delayed scaling: last forward's amax -> this one's scales
  if (train) n->packed_eval = false;               // running statistics are about to change
  TRYI(alloc_heads(n, N));
  TRYI(backbone_forward(n, train, xs, in_f32, N, H, W, E, st));
  TRYI(heads_forward(n, E, npass, N, st));
  if (feats) TRY(hipMemcpyAsync(feats, n->feats, (size_t)N * 768 * 4, hipMemcpyDeviceToDevice, st));
  if (logits) TRY(hipMemcpyAsync(logits, n->logits, (size_t)N * n->ncls * 4, hipMemcpyDeviceToDevice, st));
  n->last_N = N; n->last_npass = train ? npass : 0;
  return 0;
}

int net_backward(sslcr_net* n, const float* dlogits, hipStream_t st) {
  sslcr_ctx* c = n->ctx;
  if (n->last_npass == 0) return fail("sslcr_net_backward: no train-mode forward to differentiate");
  const int N = n->last_N, npass = n->last_npass;
  TRYI(n->grads.ensure(n->grad_count * sizeof(float)));
  // accumulating: this backward's gradient goes to the second buffer, and only over the range a backward can write
  const bool acc = n->grad_accum && n->had_backward;
  const size_t acc_lo = acc ? n->goff[lowest_trainable(n)] : 0;
  if (acc) TRYI(n->gnew.ensure(n->grad_count * sizeof(float)));
  n->gw = (float*)(acc ? n->gnew.p : n->grads.p);
  TRY(hipMemsetAsync(n->gw + acc_lo, 0, (n->grad_count - acc_lo) * sizeof(float), st));
  const bool bb = lowest_trainable(n) < 60;
  if (bb) {
    TRYI(c->bn_ring.ensure((size_t)sslcr_ctx::kBnRing * sslcr_ctx::kBnSlot * sizeof(double)));
    c->bn_ring_i = 0;
  }
  TRYI(heads_backward(n, dlogits, npass, N, bb, st));
  TRYI(launch_bucket_allreduce(n, 0, n->goff[60], n->goff[n->nparams], st));
  if (bb) {
    TRYI(backbone_backward(n, npass, st));
  }
  if (sharded(c)) {
    TRY(hipEventRecord(c->ev_done, c->comm_stream));
    TRY(hipStreamWaitEvent(st, c->ev_done, 0));
  }
  TRYI(wg_join(c, st));                       // the optimizer (and the next step's scratch writers) come after the side-stream wgrads
  c->wg_any = false;
  for (bool& pnd : c->wg_pending) pnd = false;
  if (acc) {                                   // prev + new, behind every writer of `new` (the collectives included)
    TRY(launch_grad_accumulate((float*)n->grads.p + acc_lo, n->gw + acc_lo, n->grad_count - acc_lo, st));
    n->gw = (float*)n->grads.p;
  }
  n->had_backward = true;
  return 0;
}

}  // namespace

extern "C" {

int sslcr_create(sslcr_ctx** out, int device, int dtype) {
  if (!out || (dtype != SSLCR_F32 && dtype != SSLCR_BF16 && dtype != SSLCR_FP8)) return fail("sslcr_create: invalid argument");
  TRY(hipSetDevice(device));
  sslcr_ctx* c = new sslcr_ctx();
  c->device = device; c->dtype = dtype == SSLCR_FP8 ? SSLCR_BF16 : dtype; c->fp8 = dtype == SSLCR_FP8;
  c->fuse_stem_bwd = sw::on(sw::FUSE_STEM_BWD);       // asked at every create: a test sets it between two engines of one process
  // bn_stage: [kMaxSeg][32][2][C] (sslcr_bn_finalize_desc.stage with segments)
  if (c->small.ensure((size_t)kMaxSeg * 32 * 2 * 512 * sizeof(double) + 2 * 2 * 512 * sizeof(double) + 2 * 512 * sizeof(float) + 64 * sizeof(int)) != 0) { delete c; return -1; }
  c->bn_stage = (double*)c->small.p;
  c->bn_sums = c->bn_stage + (size_t)kMaxSeg * 32 * 2 * 512;        // two [2][C] slots (bn2 + projection BatchNorm of a block share an all-reduce)
  c->ones = (float*)(c->bn_sums + 2 * 2 * 512);
  c->zeros = c->ones + 512;
  c->bn_tickets = (int*)(c->zeros + 512);
  TRY(hipMemset(c->bn_tickets, 0, 64 * sizeof(int)));
  TRY(launch_fill(c->ones, 512, 1.f, nullptr));
  TRY(launch_fill(c->zeros, 512, 0.f, nullptr));
  TRY(hipStreamSynchronize(nullptr));
  g_live_ctx.fetch_add(1);
  *out = c;
  return 0;
}

int sslcr_destroy(sslcr_ctx* c) {
  if (!c) return 0;
  (void)hipDeviceSynchronize();
  if (c->wg_stream) {
    (void)hipStreamDestroy(c->wg_stream);
    for (int k = 0; k < 3; ++k) { (void)hipEventDestroy(c->ev_wg_in[k]); (void)hipEventDestroy(c->ev_wg_done[k]); }
    (void)hipEventDestroy(c->ev_wg_join);
  }
  if (c->aux_stream) {
    (void)hipStreamDestroy(c->aux_stream);
    (void)hipEventDestroy(c->ev_aux_begin);
    (void)hipEventDestroy(c->ev_aux_end);
  }
  if (c->comm || c->vcomm) {
    if (c->comm) ncclCommDestroy(c->comm);
    if (c->comm_g) ncclCommDestroy(c->comm_g);
    (void)hipStreamDestroy(c->comm_stream);
    for (int i = 0; i < 8; ++i) (void)hipEventDestroy(c->ev_ready[i]);
    (void)hipEventDestroy(c->ev_done);
  }
  c->scratch.release(); c->partials.release(); c->small.release(); c->bn_ring.release();
  // the per-stream fold scratch of the weight-gradient / BatchNorm-backward launches is process-global: freed with the LAST live
  // context only -- another context's host thread (virtual ranks) may hold a slab pointer it has not launched with yet
  if (g_live_ctx.fetch_sub(1) == 1) stream_scratch_release();
  delete c;
  return 0;
}

int sslcr_profile(sslcr_ctx* c, int enable) {
  if (!c) return fail("sslcr_profile: null");
  c->prof.on = enable != 0;
  if (enable) {
    for (int w = 0; w < 3; ++w) {
      for (auto& r : c->prof.rec[w]) { c->prof.pool.push_back(r.e0); c->prof.pool.push_back(r.e1); }
      c->prof.rec[w].clear();
    }
  }
  return 0;
}

int sslcr_profile_dump(sslcr_ctx* c, char* buf, size_t n) {
  if (!c || !buf || n < 64) return fail("sslcr_profile_dump: invalid argument");
  TRY(hipDeviceSynchronize());
  struct Row { const char* name; double launches, ms, flops, bytes; };
  std::vector<Row> rows;
  for (int w = 0; w < 3; ++w)
    for (auto& r : c->prof.rec[w]) {
      float t = 0.f;
      TRY(hipEventElapsedTime(&t, r.e0, r.e1));
      Row* hit = nullptr;
      for (auto& q : rows)
        if (strcmp(q.name, r.name) == 0) { hit = &q; break; }
      if (!hit) { rows.push_back(Row{r.name, 0, 0, 0, 0}); hit = &rows.back(); }
      hit->launches += 1; hit->ms += t; hit->flops += r.flops; hit->bytes += r.bytes;
    }
  size_t off = 0;
  for (auto& q : rows) {
    int k = snprintf(buf + off, n - off, "%s|%.0f|%.6f|%.6e|%.6e\n", q.name, q.launches, q.ms, q.flops, q.bytes);
    if (k < 0 || (size_t)k >= n - off) return fail("sslcr_profile_dump: buffer too small");
    off += k;
  }
  buf[off] = 0;
  return 0;
}

int sslcr_profile_read(sslcr_ctx* c, int which, double* out4) {
  if (!c || !out4 || which < 0 || which > 1) return fail("sslcr_profile_read: invalid argument");
  TRY(hipDeviceSynchronize());
  double ms = 0.0, fl = 0.0, by = 0.0;
  for (auto& r : c->prof.rec[which]) {
    float t = 0.f;
    TRY(hipEventElapsedTime(&t, r.e0, r.e1));
    ms += t; fl += r.flops; by += r.bytes;
  }
  out4[0] = (double)c->prof.rec[which].size(); out4[1] = ms; out4[2] = fl; out4[3] = by;
  return 0;
}

int sslcr_comm_unique_id(void* id256) {
  if (!id256) return fail("sslcr_comm_unique_id: null");
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId is 128 bytes");
  TRYN(ncclGetUniqueId((ncclUniqueId*)id256));
  TRYN(ncclGetUniqueId((ncclUniqueId*)((char*)id256 + 128)));
  return 0;
}

int sslcr_set_aux_stream(sslcr_ctx* c, int on) {
  if (!c) return fail("sslcr_set_aux_stream: null");
  c->use_aux = on ? 1 : 0;
  return 0;
}

int sslcr_set_wgrad_stream(sslcr_ctx* c, int on) {
  if (!c) return fail("sslcr_set_wgrad_stream: null");
  c->use_wg = on ? 1 : 0;
  return 0;
}

int sslcr_set_bn_sync(sslcr_ctx* c, int on) {
  if (!c) return fail("sslcr_set_bn_sync: null");
  c->bn_sync = on ? 1 : 0;
  return 0;
}

int sslcr_comm_init(sslcr_ctx* c, const void* id256, int rank, int world) {
  if (!c || !id256 || world < 1 || rank < 0 || rank >= world) return fail("sslcr_comm_init: invalid argument");
  // world == 1 normally needs no communicator; SSLCR_COMM_SELFTEST=1 creates the two 1-rank communicators anyway so that the
  // whole collective code path (RCCL calls, side stream, events) can be exercised on a single-GPU box (tests/test_engine_gpu.py)
  if (world == 1 && !sw::on(sw::COMM_SELFTEST)) { c->rank = 0; c->world = 1; return 0; }
  TRY(hipSetDevice(c->device));
  ncclUniqueId id, idg;
  memcpy(&id, id256, sizeof(id));
  memcpy(&idg, (const char*)id256 + 128, sizeof(idg));
  TRYN(ncclCommInitRank(&c->comm, world, id, rank));
  TRYN(ncclCommInitRank(&c->comm_g, world, idg, rank));
  TRY(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
  for (int i = 0; i < 8; ++i) TRY(hipEventCreateWithFlags(&c->ev_ready[i], hipEventDisableTiming));
  TRY(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
  c->rank = rank; c->world = world;
  return 0;
}

int sslcr_comm_info(sslcr_ctx* c, int* rank, int* world, int* transport) {
  if (!c) return fail("sslcr_comm_info: null");
  int r = c->rank, w = c->world;
  if (c->comm) {                 // what RCCL itself says, not what the caller passed
    TRYN(ncclCommUserRank(c->comm, &r));
    TRYN(ncclCommCount(c->comm, &w));
  }
  if (rank) *rank = r;
  if (world) *world = w;
  if (transport) *transport = c->comm ? 1 : c->vcomm ? 2 : 0;
  return 0;
}

int sslcr_comm_all_reduce_f32(sslcr_ctx* c, float* buf, size_t n, void* stream) {
  if (!c || (!buf && n)) return fail("sslcr_comm_all_reduce_f32: invalid argument");
  if (!sharded(c) || n == 0) return 0;
  return all_reduce(c, 0, buf, n, false, (hipStream_t)stream);
}

int sslcr_vcomm_create(sslcr_vcomm** out, int world) {
  if (!out || world < 1 || world > VW_MAX) return fail("sslcr_vcomm_create: world must be 1..%d", VW_MAX);
  sslcr_vcomm* v = new sslcr_vcomm();
  v->world = world;
  *out = v;
  return 0;
}

int sslcr_vcomm_destroy(sslcr_vcomm* v) {
  if (!v) return 0;
  (void)hipDeviceSynchronize();
  for (auto& ch : v->ch)
    for (int ph = 0; ph < 2; ++ph)
      for (int q = 0; q < VW_MAX; ++q) {
        if (ch.slot[ph][q]) (void)hipFree(ch.slot[ph][q]);
        if (ch.ev_in[ph][q]) { (void)hipEventDestroy(ch.ev_in[ph][q]); (void)hipEventDestroy(ch.ev_out[ph][q]); }
      }
  delete v;
  return 0;
}

int sslcr_comm_init_virtual(sslcr_ctx* c, sslcr_vcomm* v, int rank) {
  if (!c || !v || rank < 0 || rank >= v->world) return fail("sslcr_comm_init_virtual: invalid argument");
  if (c->comm || c->vcomm) return fail("sslcr_comm_init_virtual: this context already has a communicator");
  TRY(hipSetDevice(c->device));
  TRY(hipStreamCreateWithFlags(&c->comm_stream, hipStreamNonBlocking));
  for (int i = 0; i < 8; ++i) TRY(hipEventCreateWithFlags(&c->ev_ready[i], hipEventDisableTiming));
  TRY(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
  c->vcomm = v; c->rank = rank; c->world = v->world;
  return 0;
}

int sslcr_net_create(sslcr_ctx* c, const sslcr_net_desc* d, sslcr_net** out) {
  if (!c || !d || !out || !d->params) return fail("sslcr_net_create: null");
  const int want = 64 + (d->head_kind == 0 ? 2 : 4);
  if (d->nparams != want) return fail("sslcr_net_create: expected %d parameters (64 net + classifier), got %d", want, d->nparams);
  if (d->num_classes < 1 || d->num_classes > 64) return fail("sslcr_net_create: num_classes out of range");
  sslcr_net* n = new sslcr_net();
  n->ctx = c; n->nparams = d->nparams; n->head_kind = d->head_kind; n->ncls = d->num_classes; n->triplet = d->triplet;
  n->params.assign(d->params, d->params + d->nparams);
  n->rg.assign(d->nparams, 1);
  if (d->requires_grad) n->rg.assign(d->requires_grad, d->requires_grad + d->nparams);
  for (int i = 0; i < 20; ++i) {
    n->bn_rm[i] = d->bn_running_mean[i]; n->bn_rv[i] = d->bn_running_var[i];
    n->bn_nbt[i] = d->bn_num_batches_tracked ? d->bn_num_batches_tracked[i] : nullptr;
  }
  build_topology(n);
  if (alloc_shadow(n) != 0) { delete n; return -1; }
  *out = n;
  return 0;
}

int sslcr_net_destroy(sslcr_net* n) {
  if (!n) return 0;
  (void)hipDeviceSynchronize();
  for (DevBuf* b : n->bufs()) b->release();
  delete n;
  return 0;
}

int sslcr_net_set_requires_grad(sslcr_net* n, const uint8_t* flags) {
  if (!n || !flags) return fail("sslcr_net_set_requires_grad: null");
  n->rg.assign(flags, flags + n->nparams);
  n->ndesc = 0;
  return 0;
}

int sslcr_net_pack(sslcr_net* n, int mode, void* stream) {
  if (!n || !(mode & 3)) return fail("sslcr_net_pack: invalid argument");
  hipStream_t st = (hipStream_t)stream;
  for (const Layer& ly : n->layers) TRYI(pack_conv_layer(n, *ly.conv, *ly.bn, mode, st));
  if (mode & 1) n->packed_train = true;
  if (mode & 2) n->packed_eval = true;
  // a full re-pack is what the host asks for after it changed parameters behind the engine's back (load_state_dict, --resume):
  // the fp8 activation scales were calibrated on the previous weights, so the next forward of each mode calibrates again
  if (mode == 3) n->f8_cal[0] = n->f8_cal[1] = false;
  return 0;
}

int sslcr_net_forward(sslcr_net* n, int train, const void* x1, const void* x2, const void* x3, int in_f32, int N, int H, int W,
                      float* feats, float* logits, void* stream) {
  if (!n || !x1 || N < 1 || H < 32 || W < 32) return fail("sslcr_net_forward: invalid argument");
  if (n->triplet && (!x2 || !x3)) return fail("sslcr_net_forward: TripletNet needs three inputs");
  const void* xs[3] = {x1, x2, x3};
  return net_forward(n, train, xs, in_f32, N, H, W, feats, logits, (hipStream_t)stream);
}

int sslcr_net_backward(sslcr_net* n, const float* dlogits, void* stream) {
  if (!n || !dlogits) return fail("sslcr_net_backward: null");
  return net_backward(n, dlogits, (hipStream_t)stream);
}

int sslcr_net_segments_used(const sslcr_net* n) { return (n && n->last_segments) ? 1 : 0; }
int sslcr_net_set_grad_accumulate(sslcr_net* n, int on) {
  if (!n) return fail("sslcr_net_set_grad_accumulate: null net");
  n->grad_accum = on != 0;
  return 0;
}

int sslcr_net_set_loss_opts(sslcr_net* n, const sslcr_loss_opts* o) {
  if (!n) return fail("sslcr_net_set_loss_opts: null net");
  if (o) {
    const char* why = loss_opts_error(1, n->ncls, *o);      // the ranges; what a step's kind refuses is that step's error
    if (why) return fail("sslcr_net_set_loss_opts: invalid argument (%s)", why);
  }
  n->lopts = o ? *o : loss_opts_default();
  return 0;
}
// the loss leg of the step entries: launch_loss itself unless the net carries options
static int step_loss(sslcr_net* n, const LossArgs& L, const char* who, hipStream_t st) {
  if (loss_opts_is_default(n->lopts)) {
    TRY(launch_loss(L, st));
    return 0;
  }
  const char* why = loss_opts_error(L.kind, L.C, n->lopts);
  if (why) return fail("%s: %s (sslcr_net_set_loss_opts)", who, why);
  TRY(launch_loss_ex(L, n->lopts, st));
  return 0;
}

int sslcr_net_debug_tap(sslcr_net* n, int on) {
  if (!n) return fail("sslcr_net_debug_tap: null net");
  n->tap = on != 0;
  if (!on)
    for (auto& ps : n->tapbuf)
      for (auto& row : ps)
        for (DevBuf& b : row) b.release();
  return 0;
}

int sslcr_net_debug_tensor(sslcr_net* n, int block, int kind, void* out, size_t out_bytes, int* dims4, int* flags, void* stream) {
  const int pass = kind >> 8;         // the pass rides in the high bits: kind | pass << 8
  kind &= 0xff;
  if (!n || block < 0 || block > 7 || pass < 0 || pass > 2 || kind > 29 || !dims4) return fail("sslcr_net_debug_tensor: invalid argument");
  sslcr_ctx* c = n->ctx;
  hipStream_t st = (hipStream_t)stream;
  const BlockL& B = n->blocks[block];
  if (n->last_npass == 0 || !n->pass[0].mem.p) return fail("sslcr_net_debug_tensor: no train-mode forward");
  if (pass >= n->last_npass) return fail("sslcr_net_debug_tensor: pass %d of a forward with %d", pass, n->last_npass);
  const PassState& ps = n->pass[pass];
  const Dims d = make_dims(ps.H, ps.W);
  const int oh = d.lh[block], ow = d.lw[block];
  const int xh = block == 0 ? d.ph : d.lh[block - 1], xw = block == 0 ? d.pw : d.lw[block - 1];
  const void* src = nullptr;
  size_t esz = c->esz();
  int dm[4] = {ps.N, oh, ow, B.c2.cout};
  if (kind <= 5 || kind == 29) {
    const int slot = kind == 29 ? 6 : kind;
    if (!n->tap || !n->tapbuf[pass][block][slot].p)
      return fail("sslcr_net_debug_tensor: nothing tapped for block %d kind %d pass %d", block, kind, pass);
    src = n->tapbuf[pass][block][slot].p;
    for (int j = 0; j < 4; ++j) dm[j] = n->tapdims[pass][block][slot][j];
  } else if (kind == 6) { src = ps.blk[block].raw1; dm[3] = B.c1.cout; }
  else if (kind == 7) { src = ps.blk[block].raw2; }
  else if (kind == 8) { src = ps.blk[block].rawd; if (!B.has_ds) return fail("sslcr_net_debug_tensor: block %d has no projection", block); }
  else if (kind == 9) { src = ps.blk[block].y; }
  else if (kind == 10) { src = block == 0 ? ps.pooled : ps.blk[block - 1].y; dm[1] = xh; dm[2] = xw; dm[3] = B.c1.cin; }
  else if (kind >= 15 && kind <= 20) {   // the train-mode shadow weights of conv1, conv2, the projection: forward pack, dgrad pack
    const ConvL& L = kind < 17 ? B.c1 : kind < 19 ? B.c2 : B.ds;
    if (kind >= 19 && !B.has_ds) return fail("sslcr_net_debug_tensor: block %d has no projection", block);
    const bool fwd = (kind & 1) != 0;
    src = fwd ? L.w_fwd : L.w_dg;
    if (!src) return fail("sslcr_net_debug_tensor: block %d kind %d: this conv has no such pack", block, kind);
    dm[0] = fwd ? L.cout : L.cin; dm[1] = dm[2] = L.k; dm[3] = fwd ? L.cin : L.cout;
  } else {                      // 11..14, 21..24, 25..28: the saved scale, shift, mean, invstd of bn1, bn2, the projection's BatchNorm (fp32 [C])
    const BnL& bn = kind <= 14 ? B.b1 : kind <= 24 ? B.b2 : B.bd;
    if (kind >= 25 && !B.has_ds) return fail("sslcr_net_debug_tensor: block %d has no projection", block);
    const BnSaved& sv = ps.bn[bn.bidx];
    const float* v[4] = {sv.scale, sv.shift, sv.mean, sv.invstd};
    src = v[kind <= 14 ? kind - 11 : kind <= 24 ? kind - 21 : kind - 25]; esz = 4; dm[0] = bn.C; dm[1] = dm[2] = dm[3] = 1;
  }
  for (int j = 0; j < 4; ++j) dims4[j] = dm[j];
  if (flags) *flags = n->tap_flags[block] | n->fwd_flags[block];
  if (!out) return 0;
  const size_t bytes = (size_t)dm[0] * dm[1] * dm[2] * dm[3] * esz;
  if (out_bytes < bytes) return fail("sslcr_net_debug_tensor: buffer of %zu bytes, tensor has %zu", out_bytes, bytes);
  TRY(hipMemcpyAsync(out, src, bytes, hipMemcpyDeviceToDevice, st));
  return 0;
}

int sslcr_net_grad(sslcr_net* n, int pidx, float* out, void* stream) {
  if (!n || !out || pidx < 0 || pidx >= n->nparams) return fail("sslcr_net_grad: invalid argument");
  if (!n->grads.p) return fail("sslcr_net_grad: no backward has run");
  hipStream_t st = (hipStream_t)stream;
  const float* g = (const float*)n->grads.p + n->goff[pidx];
  if (const ConvL* L = n->block_conv[pidx]) {
    TRY(launch_unpack_grad(g, out, L->cout, L->cin, L->k * L->k, st));
  } else {
    TRY(hipMemcpyAsync(out, g, (size_t)n->psize[pidx] * 4, hipMemcpyDeviceToDevice, st));
  }
  return 0;
}

// the flat gradient buffer holds exactly what sslcr_net_grad exposes for the trainable parameters and zeros elsewhere (frozen
// parameters' ranges, the padding to 64 elements behind every parameter): net_backward clears it and only trainable parameters'
// ranges are written, each with exactly psize elements -- so ONE reduction over [0, grad_count) is the global norm
int net_grad_norm(sslcr_net* n, float max_norm, float* out2, hipStream_t st) {
  TRYI(n->norm_ws.ensure(GRAD_NORM_BLOCKS * sizeof(double) + 2 * sizeof(float)));
  double* partials = (double*)n->norm_ws.p;
  TRY(launch_grad_norm((const float*)n->grads.p, n->grad_count, max_norm, partials, out2 ? out2 : (float*)(partials + GRAD_NORM_BLOCKS), st));
  return 0;
}

int sslcr_net_grad_norm(sslcr_net* n, float max_norm, float* out2, void* stream) {
  if (!n || !out2) return fail("sslcr_net_grad_norm: null");
  if (!n->grads.p) return fail("sslcr_net_grad_norm: no gradients (run a backward first)");
  if (max_norm < 0.f) return fail("sslcr_net_grad_norm: max_norm must not be negative");
  return net_grad_norm(n, max_norm, out2, (hipStream_t)stream);
}

int sslcr_net_optimizer_step(sslcr_net* n, const sslcr_opt_desc* o, float* const* s1, float* const* s2, void* stream) {
  if (!o) return fail("sslcr_net_optimizer_step: null");
  return sslcr_net_optimizer_step_groups(n, o, 1, nullptr, s1, s2, nullptr, stream);
}

int sslcr_net_optimizer_step_groups(sslcr_net* n, const sslcr_opt_desc* groups, int ngroups, const int* group_of, float* const* s1,
                                    float* const* s2, const sslcr_clip_desc* clip, void* stream) {
  if (!n || !groups || !s1) return fail("sslcr_net_optimizer_step: null");
  if (ngroups < 1 || ngroups > SSLCR_MAX_OPT_GROUPS) return fail("sslcr_net_optimizer_step: %d param groups (1..%d are served)", ngroups, SSLCR_MAX_OPT_GROUPS);
  if (!n->grads.p) return fail("sslcr_net_optimizer_step: no gradients (run a backward first)");
  if (clip && clip->max_norm < 0.f) return fail("sslcr_net_optimizer_step: max_norm must not be negative");
  OptTable tab = opt_table_noop();
  for (int g = 0; g < ngroups; ++g) {
    if (groups[g].kind < 0 || groups[g].kind > 2) return fail("sslcr_net_optimizer_step: group %d has kind %d (0 adam, 1 sgd-nesterov, 2 adamw)", g, groups[g].kind);
    tab.row[g] = groups[g];
  }
  for (int i = 0; i < n->nparams; ++i) {
    const int g = group_of ? group_of[i] : 0;
    if (n->rg[i] && (g < 0 || g >= ngroups)) return fail("sslcr_net_optimizer_step: parameter %d is in group %d of %d", i, g, ngroups);
  }
  hipStream_t st = (hipStream_t)stream;
  // clipping: norm and coefficient stay on the device; the update reads the coefficient once per workgroup.  (In front of the
  // early returns below: with nothing trainable the caller still gets {0, 1}.)
  const float* coef = nullptr;
  if (clip) {
    TRYI(net_grad_norm(n, clip->max_norm, clip->out2, st));
    coef = (clip->out2 ? clip->out2 : (const float*)((const double*)n->norm_ws.p + GRAD_NORM_BLOCKS)) + 1;
  }
  // (re)build the device descriptor table when the state pointers, the trainable set or the group map changed
  bool rebuild = n->ndesc == 0 || (int)n->st1.size() != n->nparams;
  if (!rebuild)
    for (int i = 0; i < n->nparams; ++i)
      if (n->st1[i] != s1[i] || n->st2[i] != (s2 ? s2[i] : nullptr) || (n->rg[i] && n->group_of[i] != (group_of ? group_of[i] : 0))) {
        rebuild = true;
        break;
      }
  if (rebuild) {
    n->host_descs.clear();
    n->max_n = 0;
    std::vector<int2> host_chunks;
    int packed_convs = 0;
    for (int i = 0; i < n->nparams; ++i) {
      if (!n->rg[i]) continue;
      const int grp = group_of ? group_of[i] : 0;
      if (!s1[i] || (groups[grp].kind != 1 && (!s2 || !s2[i]))) return fail("sslcr_net_optimizer_step: missing optimizer state for parameter %d", i);
      sslcr_tensor_desc t;
      memset(&t, 0, sizeof(t));
      t.group = grp;
      t.p = n->params[i]; t.g = (float*)n->grads.p + n->goff[i]; t.s1 = s1[i]; t.s2 = s2 ? s2[i] : nullptr; t.n = n->psize[i];
      if (const ConvL* L = n->block_conv[i]) {
        t.K = L->cout; t.C = L->cin; t.RS = L->k * L->k;
        // the update writes the train-mode shadow weights of the new value (what pack_conv_layer(mode 1) would produce)
        t.w_fwd = L->w_fwd; t.w_dgrad = L->w_dg; t.pack_dtype = n->ctx->dtype; t.dgrad_flip = (L->k == 3 && L->stride == 1);
        ++packed_convs;
      }
      // work list: OPT_CHUNK elements per entry
      const int ti = (int)n->host_descs.size() | (t.group << OPT_CHUNK_GROUP_SHIFT);      // the chunk repeats the group (optim.hip)
      if (t.K > 0 && t.RS == 9 && t.w_fwd && t.w_dgrad && t.K % 16 == 0 && t.C % 16 == 0) {
        for (int tile = 0; tile < (t.K / 16) * (t.C / 16); ++tile) host_chunks.push_back({ti, -(tile + 1)});   // LDS-transposed tiles
      } else {
        for (int e = 0; e < t.n; e += OPT_CHUNK) host_chunks.push_back({ti, e});
      }
      n->host_descs.push_back(t);
      if (t.n > n->max_n) n->max_n = t.n;
    }
    n->ndesc = (int)n->host_descs.size();
    if (n->ndesc == 0) return 0;
    n->opt_packs_all = packed_convs == kLayers - 1;      // (every layer but the stem)
    n->nchunks = (int)host_chunks.size();
    TRYI(n->chunks.ensure(host_chunks.size() * sizeof(int2)));
    TRY(hipMemcpyAsync(n->chunks.p, host_chunks.data(), host_chunks.size() * sizeof(int2), hipMemcpyHostToDevice, st));
    TRYI(n->descs.ensure(n->ndesc * sizeof(sslcr_tensor_desc)));
    TRY(hipMemcpyAsync(n->descs.p, n->host_descs.data(), n->ndesc * sizeof(sslcr_tensor_desc), hipMemcpyHostToDevice, st));
    TRY(hipStreamSynchronize(st));       // host_descs may be rebuilt before the copy would otherwise land
    n->st1.assign(s1, s1 + n->nparams);
    if (s2) n->st2.assign(s2, s2 + n->nparams); else n->st2.assign(n->nparams, nullptr);
    n->group_of.assign(n->nparams, 0);
    if (group_of) n->group_of.assign(group_of, group_of + n->nparams);
  }
  if (n->ndesc == 0) return 0;
  // sharded runs: every rank's loss is already scaled by 1/(global batch), so the all-reduced SUM is the exact gradient
  TRY(launch_optimizer_chunks((const sslcr_tensor_desc*)n->descs.p, n->chunks.p, n->nchunks, tab, coef, st));
  n->packed_train = false; n->packed_eval = false;
  if (n->opt_packs_all) {
    // every block conv's shadow weights were rewritten with the update; only the stem's (its own K order) are left
    TRYI(pack_conv_layer(n, n->stem, n->bn0, 1, st));
    // e4m3 train packs of the updated filters (the bf16 packs were written by the update itself)
    for (const Layer& ly : n->layers) TRYI(pack_fp8_layer(n, *ly.conv, *ly.bn, 1, st));
    n->packed_train = true;
  }
  return 0;
}

int sslcr_net_lookahead(sslcr_net* n, float* const* cached, float alpha, void* stream) {
  if (!n || !cached) return fail("sslcr_net_lookahead: null");
  for (int i = 0; i < n->nparams; ++i)
    if (cached[i]) TRY(launch_axpby(n->params[i], cached[i], n->psize[i], alpha, 1, (hipStream_t)stream));
  n->packed_train = false; n->packed_eval = false;
  return 0;
}

int sslcr_net_ema_from(sslcr_net* t, sslcr_net* s, float decay, void* stream) {
  if (!t || !s || t->nparams != s->nparams) return fail("sslcr_net_ema_from: mismatched nets");
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < t->nparams; ++i) TRY(launch_axpby(t->params[i], s->params[i], t->psize[i], decay, 0, st));
  // BN buffers are copied (deepcopy semantics for running statistics)
  for (const Layer& ly : t->layers) {
    const int b = ly.bn->bidx, bytes = ly.bn->C * 4;
    TRY(hipMemcpyAsync(t->bn_rm[b], s->bn_rm[b], bytes, hipMemcpyDeviceToDevice, st));
    TRY(hipMemcpyAsync(t->bn_rv[b], s->bn_rv[b], bytes, hipMemcpyDeviceToDevice, st));
    if (t->bn_nbt[b] && s->bn_nbt[b]) TRY(hipMemcpyAsync(t->bn_nbt[b], s->bn_nbt[b], 8, hipMemcpyDeviceToDevice, st));
  }
  t->packed_train = false; t->packed_eval = false;
  return 0;
}

int sslcr_step_ssl_cr(sslcr_net* te, sslcr_net* stn, const sslcr_ssl_cr_desc* d, void* stream) {
  if (!te || !stn || !d || !d->x_student || !d->x_teacher || !d->losses) return fail("sslcr_step_ssl_cr: null");
  if (d->nx < 1 || d->nu < 1) return fail("sslcr_step_ssl_cr: nx, nu must be positive");
  if (te->ncls != stn->ncls) return fail("sslcr_step_ssl_cr: teacher/student class count differ");
  hipStream_t st = (hipStream_t)stream;
  const int Ns = d->nx + d->nu;
  TRYI(alloc_heads(stn, Ns));
  // teacher: eval + no_grad (eval_BreastPathQ_SSL_CR.py:43-44,77-79) -- on the second stream when sslcr_set_aux_stream asked
  // for it (the per-kernel profiler records each launch on the stream it runs on)
  sslcr_ctx* c = stn->ctx;
  const bool aux = c->use_aux && te->ctx == c && !c->prof.on;     // (per-kernel profiling: serialised, like the weight-gradient stream)
  hipStream_t tst = st;
  if (aux) {
    if (!c->aux_stream) {
      TRY(hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));
      TRY(hipEventCreateWithFlags(&c->ev_aux_begin, hipEventDisableTiming));
      TRY(hipEventCreateWithFlags(&c->ev_aux_end, hipEventDisableTiming));
    }
    TRY(hipEventRecord(c->ev_aux_begin, st));                 // inputs ready, last step's backward done with the scratch
    TRY(hipStreamWaitEvent(c->aux_stream, c->ev_aux_begin, 0));
    tst = c->aux_stream;
  }
  const void* xt[3] = {d->x_teacher, nullptr, nullptr};
  TRYI(net_forward(te, 0, xt, d->in_f32, d->nu, d->H, d->W, nullptr, stn->logits_t, tst));
  if (aux) TRY(hipEventRecord(c->ev_aux_end, c->aux_stream));
  // student: train mode on cat(x, u_s) (:82-84)
  const void* xs[3] = {d->x_student, nullptr, nullptr};
  if (d->x_student2 && stn->triplet) return fail("sslcr_step_ssl_cr: split student input needs a single-branch net");
  stn->split_x2 = d->x_student2; stn->split_n = d->nx;
  const int frc = net_forward(stn, 1, xs, d->in_f32, Ns, d->H, d->W, d->feats, d->logits, st);
  stn->split_x2 = nullptr; stn->split_n = 0;
  if (frc) return frc;
  if (aux) TRY(hipStreamWaitEvent(st, c->ev_aux_end, 0));
  LossArgs L;
  memset(&L, 0, sizeof(L));
  L.kind = d->kind; L.logits = stn->logits; L.logits_t = stn->logits_t; L.target_f = d->target_f; L.target_i = d->target_i;
  L.dlogits = d->backward ? stn->dlogits : nullptr; L.out = d->losses; L.nx = d->nx; L.nu = d->nu; L.C = stn->ncls; L.lambda_u = d->lambda_u;
  L.inv_nx_global = 1.f / (float)(d->nx_global > 0 ? d->nx_global : d->nx);
  L.inv_nu_global = 1.f / (float)(d->nu_global > 0 ? d->nu_global : d->nu);
  if (d->kind == 0 && !d->target_f) return fail("sslcr_step_ssl_cr: mse needs target_f");
  if (d->kind == 1 && !d->target_i) return fail("sslcr_step_ssl_cr: ce needs target_i");
  TRYI(step_loss(stn, L, "sslcr_step_ssl_cr", st));
  if (d->logits_t) TRY(hipMemcpyAsync(d->logits_t, stn->logits_t, (size_t)d->nu * stn->ncls * 4, hipMemcpyDeviceToDevice, st));
  if (d->backward) TRYI(net_backward(stn, stn->dlogits, st));
  return 0;
}

int sslcr_step_supervised(sslcr_net* n, const sslcr_sup_desc* d, void* stream) {
  if (!n || !d || !d->x1 || !d->losses) return fail("sslcr_step_supervised: null");
  if (d->kind != 2 && d->kind != 3) return fail("sslcr_step_supervised: kind must be 2 (ce) or 3 (mse)");
  if (n->triplet && (!d->x2 || !d->x3)) return fail("sslcr_step_supervised: TripletNet needs three inputs");
  hipStream_t st = (hipStream_t)stream;
  const void* xs[3] = {d->x1, d->x2, d->x3};
  TRYI(net_forward(n, d->train, xs, d->in_f32, d->n, d->H, d->W, d->feats, d->logits, st));
  LossArgs L;
  memset(&L, 0, sizeof(L));
  L.kind = d->kind; L.logits = n->logits; L.target_f = d->target_f; L.target_i = d->target_i;
  L.dlogits = (d->train && d->backward) ? n->dlogits : nullptr; L.out = d->losses; L.nx = d->n; L.nu = 0; L.C = n->ncls;
  L.inv_nx_global = 1.f / (float)(d->n_global > 0 ? d->n_global : d->n); L.inv_nu_global = 1.f;
  if (d->kind == 3 && !d->target_f) return fail("sslcr_step_supervised: mse needs target_f");
  if (d->kind == 2 && !d->target_i) return fail("sslcr_step_supervised: ce needs target_i");
  TRYI(step_loss(n, L, "sslcr_step_supervised", st));
  if (d->train && d->backward) TRYI(net_backward(n, n->dlogits, st));
  return 0;
}

}  // extern "C"

// The switch table (switches.hpp) and the only getenv("SSLCR_...") of csrc/: read() below, through the row's name
// (tests/test_switch_routes_cpu.py walks the sources for a second one).
#include "switches.hpp"

#include <limits.h>
#include <stdlib.h>

#include <array>

namespace sslcr {
namespace sw {
namespace {

#define ON(id, rule, when, group, meaning) {id, "SSLCR_" #id, rule, 1, 0, 1, when, group, meaning}
#define OFF(id, rule, when, group, meaning) {id, "SSLCR_" #id, rule, 0, 0, 1, when, group, meaning}
#define NUM(id, dflt, lo, hi, group, meaning) {id, "SSLCR_" #id, INT, dflt, lo, hi, PROCESS, group, meaning}
constexpr Row kRows[] = {
    ON(PP64, ATOI, PROCESS, "routing", "bf16 64 -> 64 3x3 convs on conv3x3_pp64_kernel; 0: conv3x3_h16's resident-filter form keeps them"),
    ON(H16_TW8, ATOI, PROCESS, "routing", "8x8 maps as four-image tiles of conv3x3_h16 (128-kout blocks); 0: conv3x3_halo256 keeps the shape"),
    ON(H16_RAW, ATOI, PROCESS, "routing", "the train-mode forward's output stage of conv3x3_h16 (the RAW instance); 0: the general body"),
    ON(S2, ATOI, PROCESS, "routing", "the 3x3 / 2 forward on conv_s2_kernel; 0: the gather kernel keeps these shapes"),
    ON(S2D, ATOI, PROCESS, "routing", "the stride-2 input gradient on conv_s2d_kernel (par4); 0: the gather kernel keeps the shape"),
    ON(S2W, ATOI, PROCESS, "routing", "the 3x3 / 2 weight gradient on wgrad_s2_kernel; 0: the gather kernel (wgrad_kernel) keeps the shape"),
    ON(WG_DMA, ATOI, PROCESS, "routing", "the 3x3 / 1 weight gradient of 128-kout blocks on wgrad3x3_dma_kernel; 0: wgrad3x3_halo_kernel"),
    ON(WGRAD_WIDE, LEAD0, PROCESS, "routing", "bf16 weight gradients with K % 128 == 0 on the 128-kout wgrad_kernel<.., 2>; off: the 64-kout instance"),
    ON(GEMM_LDS, ATOI, PROCESS, "form", "the heads' GEMM through LDS where the shape allows; 0: the direct-fetch form for everything"),
    NUM(STEM_POOL_FORM, 2, INT_MIN, INT_MAX, "form", "conv1's weight gradient from the pooled gradient: 2 the role-split kernel (bf16), 1 the single-role kernel in bf16 mode too"),
    OFF(POOL_BANDS, ATOI, PROCESS, "form", "the max-pool row kernels walk their rows in eight bands; off: measured +0.07 ms per step (15.39 -> 15.46 ms, three alternations)"),
    NUM(WG_STAGGER, 1, INT_MIN, INT_MAX, "form", "wgrad3x3_dma_kernel spreads the next tile's nine DMA requests over the MFMA loop; 0: all nine in front of it (+0.14 ms per step)"),
    ON(SEGMENTS, LEAD0, PROCESS, "engine", "the TripletNet branches as segments of one launch per layer; off: pass by pass"),
    ON(BN_PAIR, ATOI, PROCESS, "engine", "bn2 and the projection BatchNorm of a downsampling block share one backward reduce / apply pair; 0: two passes each"),
    ON(BN_PAIR_G, ATOI, PROCESS, "engine", "the paired reduce writes g = dOut * (y > 0); 0: the apply pass forms it again from dOut and the mask bits (15.81 -> 15.90 ms same box)"),
    ON(YBITS, ATOI, PROCESS, "engine", "bf16: the ReLU mask of a block output as bits for bn2's backward reduce; 0: it reads the saved tensor"),
    ON(UNFOLD_EVAL, ATOI, PROCESS, "engine", "bf16: eval-mode BatchNorm scale in the conv epilogues, not in the filters; 0: folded (tools/bf16_teacher_fold_experiment.py)"),
    ON(STEM_POOL, ATOI, PROCESS, "engine", "bf16 eval: conv1 + ReLU + max-pool in one launch; 0: the stem and pool kernels"),
    OFF(BN_ONE_LAUNCH, ATOI, PROCESS, "engine", "with tickets the BatchNorm row reduction finalizes in the same launch; off: 4.35 us for the pair against 5.9 us (profiles/r06_bn_one_launch_ab.txt)"),
    ON(FUSE_STEM_BWD, ATOI, CALL, "engine", "read by every sslcr_create: conv1's weight gradient derives dY from the pooled gradient in LDS; 0: apply pass + weight gradient"),
    OFF(COMM_SELFTEST, PRESENT, CALL, "engine", "read by every sslcr_comm_init: world == 1 creates its two 1-rank communicators anyway (the collective code path on one GPU)"),
    NUM(BN_REPEAT, 1, 1, INT_MAX, "measurement", "MEASUREMENT ONLY, the running statistics take n updates: every BatchNorm finalize is launched n times back to back"),
    NUM(EW_CAP, 0, 256, 65535, "measurement", "workgroups of the grid-stride elementwise launches, held to [256, 65535]; unset (0 here): three per CU, decided at the site"),
};
#undef ON
#undef OFF
#undef NUM

constexpr bool in_enum_order() {
  for (int i = 0; i < COUNT; ++i)
    if (kRows[i].id != i) return false;
  return true;
}
static_assert(sizeof(kRows) / sizeof(kRows[0]) == COUNT && in_enum_order(), "one row per sw::Id, in the enum's order");

Value read(const Row& r) {
  const char* e = getenv(r.name);
  if (!e) return {false, r.dflt};
  switch (r.rule) {
    case ATOI: return {true, atoi(e) != 0};
    case LEAD0: return {true, e[0] != '0'};
    case PRESENT: return {true, 1};
    case INT: break;
  }
  const long v = r.id == EW_CAP ? strtol(e, nullptr, 10) : atoi(e);      // (EW_CAP is held to its range before any narrowing)
  return {true, v < r.lo ? r.lo : v > r.hi ? r.hi : v};
}

}  // namespace

const Row& row(int i) { return kRows[i]; }

Value get(Id id) {
  static const std::array<Value, COUNT> once = [] {      // thread-safe: virtual ranks launch from several host threads
    std::array<Value, COUNT> a;
    for (int i = 0; i < COUNT; ++i) a[i] = read(kRows[i]);
    return a;
  }();
  return kRows[id].when == CALL ? read(kRows[id]) : once[id];
}

}  // namespace sw
}  // namespace sslcr

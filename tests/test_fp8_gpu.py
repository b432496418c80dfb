"""fp8 (OCP e4m3) forward conv path -- BASELINE config 5 (eval_Camelyon_SSL_CR.py:33-157 "fp8 MFMA conv path").

Kernel level: the HIP kernel (v_mfma_scale_f32_16x16x128_f8f6f4) against a CPU emulation of the SAME quantisation
(oracle/kernels_ref.py: activations and weights rounded to e4m3 exactly like the kernel does, fp32 convolution) -- that pins
layout, quantisation, dequantisation, epilogue and statistics; the tolerance is the bf16 rounding of the stored output.
Engine level: the drop-in Camelyon SSL_CR train() in the fp8 engine mode against the REFERENCE goldens with the measured,
stated fp8 error (north_star: "tolerance measured, not 1e-3")."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cases as C  # noqa: E402
from oracle import kernels_ref as R  # noqa: E402

from _util import held, load_golden, rel_err  # noqa: E402
from test_kernels_gpu import DEV, close, rnd  # noqa: E402

FP8_CASES = [(2, 16, 16, 128, 128), (3, 32, 32, 128, 128), (2, 16, 16, 256, 256), (8, 8, 8, 512, 512), (4, 8, 8, 256, 128),
             (70, 32, 32, 128, 128),       # 280 tiles on 256 persistent workgroups: the tile walk + cross-tile halo prefetch
             (3, 16, 32, 256, 384)]


def _bf(t):
    return t.to(torch.bfloat16).float()


@pytest.mark.parametrize("case", FP8_CASES)
def test_pack_fp8_matches_the_oracle_quantiser(case):
    from ssl_cr_histo_amd import kernels as K
    _, _, _, Cc, Ko = case
    w = rnd(11, (Ko, Cc, 3, 3), 0.05)
    w[1] *= 37.0                                      # channels of very different magnitude: per-kout scales
    w[2] *= 1e-3
    w8, dq, _ = K.pack_conv_fp8(w.to(DEV))
    wq, dq_ref, _ = R.fp8_weight_pack(w)
    got = w8.view(torch.float8_e4m3fn).float().cpu().permute(0, 3, 1, 2)           # [K,3,3,C] -> [K,C,3,3]
    assert torch.equal(dq.cpu(), dq_ref)
    assert torch.equal(got, wq)
    assert float((got.abs().flatten(1).max(1).values).min()) > 224.0 - 1e-3
    bn = tuple(t.to(DEV) for t in (rnd(12, (Ko,)).abs() + 0.5, rnd(13, (Ko,)), rnd(14, (Ko,)), rnd(15, (Ko,)).abs() + 0.5))
    w8f, dqf, bias = K.pack_conv_fp8(w.to(DEV), bn=bn)
    wqf, dqf_ref, bias_ref = R.fp8_weight_pack(w, bn=tuple(t.cpu() for t in bn))
    assert torch.equal(dqf.cpu(), dqf_ref)
    gotf = w8f.view(torch.float8_e4m3fn).float().cpu().permute(0, 3, 1, 2)
    assert float((gotf != wqf).float().mean()) < 1e-4          # w * gamma / sqrt(var + eps): one fp32 ulp can flip an e4m3 rounding
    close(bias, bias_ref, 1e-6, "folded bias")


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("case", FP8_CASES)
def test_conv_fp8_vs_quantised_oracle(case, mode):
    from ssl_cr_histo_amd import kernels as K
    N, H, W, Cc, Ko = case
    x = _bf(rnd(21, (N, H, W, Cc), 1.5) + 0.3)
    w = rnd(22, (Ko, Cc, 3, 3), 0.04)
    w8, dq, _ = K.pack_conv_fp8(w.to(DEV))
    wq, dq_ref, _ = R.fp8_weight_pack(w)
    xd = x.to(DEV).to(torch.bfloat16)
    if mode == "train":                               # producer BatchNorm + ReLU on the load path, raw output + statistics
        sc, sh = rnd(23, (Cc,)).abs() + 0.5, rnd(24, (Cc,), 0.5)
        y, stats = K.conv2d_fp8(xd, w8, dq, in_scale=sc.to(DEV), in_shift=sh.to(DEV), in_relu=True, want_stats=True)
        want, raw = R.conv3x3_fp8(x, wq, dq_ref, in_scale=sc, in_shift=sh, in_relu=True)
        close(y, want, 1.2e-2, "fp8 conv raw")
        s, ss = R.channel_stats(raw)
        st = stats.double().sum(0).cpu()
        close(st[0], s, 2e-3, "sum")
        close(st[1], ss, 2e-3, "sumsq")
    else:                                             # folded BatchNorm bias + residual + ReLU
        bias = rnd(25, (Ko,))
        res = _bf(rnd(26, (N, H, W, Ko)))
        y = K.conv2d_fp8(xd, w8, dq, bias=bias.to(DEV), residual=res.to(DEV).to(torch.bfloat16), relu=True)
        want, _ = R.conv3x3_fp8(x, wq, dq_ref, bias=bias, residual=res, relu=True)
        close(y, want, 1.2e-2, "fp8 conv eval")
    # ... and the quantisation error itself, against the un-quantised convolution of the same operands (reported, loosely bounded)
    full = R.conv_fwd(x if mode == "eval" else torch.relu(x * sc + sh), R.krsc(w), 1, 1)
    got_raw = (y.float().cpu() if mode == "train" else None)
    if got_raw is not None:
        e = float((got_raw - full).norm() / full.norm())
        print(f"fp8 vs fp32 conv, relative L2 error of the raw output: {e:.3e}")
        assert e < 6e-2


def test_conv_fp8_x_scale_and_saturation():
    """x_scale moves the activations inside the e4m3 window and is divided out again; values beyond +-448 / x_scale saturate
    (v_cvt_pk_fp8_f32 itself would produce NaN there)."""
    from ssl_cr_histo_amd import kernels as K
    N, H, W, Cc, Ko = 2, 16, 16, 128, 128
    x = _bf(rnd(31, (N, H, W, Cc), 0.01))
    x[0, 3, 3, :8] = 1000.0
    w = rnd(32, (Ko, Cc, 3, 3), 0.04)
    w8, dq, _ = K.pack_conv_fp8(w.to(DEV))
    wq, dq_ref, _ = R.fp8_weight_pack(w)
    for xs in (1.0, 16.0, 0.25):
        amax = torch.zeros(1, device=DEV)
        y = K.conv2d_fp8(x.to(DEV).to(torch.bfloat16), w8, dq, x_scale=xs, amax_out=amax)
        want, _ = R.conv3x3_fp8(x, wq, dq_ref, x_scale=xs)
        assert torch.isfinite(y.float()).all()
        close(y, want, 1.2e-2, f"x_scale {xs}")
        assert abs(float(amax) - 1000.0) <= 4.0, float(amax)        # the amax the delayed scaling feeds on: before scale and clamp (bf16: 1000)


def test_conv_fp8_rejects_unserved_shapes():
    from ssl_cr_histo_amd import kernels as K, _lib as L
    x = torch.zeros((2, 16, 16, 64), dtype=torch.bfloat16, device=DEV)
    w8 = torch.zeros((64, 3, 3, 64), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.SslcrError):
        K.conv2d_fp8(x, w8, torch.ones(64, device=DEV))


# ------------------------------------------------------------------------------------------------ engine level
def _fp8_engine():
    from test_engine_gpu import _engine
    return _engine("fp8")


def test_fp8_camelyon_full_size_step_vs_reference():
    """One Camelyon SSL_CR iteration (eval_Camelyon_SSL_CR.train: CE + hard pseudo-label CE, SGD-Nesterov, the reference's three
    randperm shuffles) at student 640 / teacher 448 images of 256x256 in the fp8 engine mode -- e4m3 forward convs in layers 2-4
    of teacher and student, bf16 everything else and the whole backward -- against the REFERENCE's golden of that iteration.
    north_star: "fp8 ... tolerance measured, not 1e-3".  Measured on MI355X: losses within 2e-2 of the reference's, feature row
    norms within 0.2 (bf16 mode: 6e-2 / 0.2); asserted at those bounds."""
    from ssl_cr_histo_amd import steps
    from test_engine_gpu import build, freeze, ns
    _fp8_engine()
    name = "cam_cr_full"
    c = C.CASES[name]
    g = load_golden(name)
    mt, ct = build("finetune", "finetune", 2, True)
    ms, cs = build("finetune", "finetune", 2, True)
    freeze(mt, 64)
    freeze(ms, c["modules"])
    opt = torch.optim.SGD(filter(lambda p: p.requires_grad, list(ms.parameters()) + list(cs.parameters())), lr=c["lr"], momentum=0.9,
                          weight_decay=c["wd"], nesterov=True)
    torch.manual_seed(777)
    ret = steps.cam_cr_train(ns(lambda_u=c["lambda_u"], image_size=c["hw"]), mt, ms, ct, cs,
                             C.labeled_batches_cls(name, 1000, 1), C.labeled_batches_cls(name, 1100, 0),
                             C.unlabeled_batches(name, 2000), C.unlabeled_batches(name, 2100), opt, 1)
    dev = [abs(ret[i] - g[f"{name}/ret"][i]) / abs(g[f"{name}/ret"][i]) for i in range(3)]
    f = ret[4].cpu().double()
    e_row = rel_err(f.norm(dim=1), g[f"{name}/feats_rowl2"])
    print(f"[fp8] Camelyon full-size step vs the reference: loss deviations {dev}, accuracy {ret[3]} vs {g[f'{name}/ret'][3]}, "
          f"feature row-norm error {e_row:.3e}")
    # 2 x the deviations measured on the MI355X (tests/measured_errors.json), ceilings 6e-2 / 0.25
    for i, d_ in enumerate(dev):
        held(f"{name}/ret{i}/fp8", d_, 6e-2, floor=2e-3)
    held(f"{name}/feats_rowl2/fp8", e_row, 0.25, floor=2e-3)
    assert torch.equal(ret[5].cpu(), torch.from_numpy(g[f"{name}/targets"]))


# ------------------------------------------------------------------------------------------------ config 5 at its own shape vs the oracle
_C5 = {}


def _config5_oracle():
    """ONE eval_Camelyon_SSL_CR.train iteration at BASELINE config 5's per-GPU shape (student 768 + 1792 = 2560, teacher 1792 images
    of 256x256) on the CPU oracle (oracle/steps.py:ssl_cr_step, one backbone pass per image).  The reference's own train() cannot
    produce this golden in the build container: TripletNet_Finetune runs the backbone three times on the 2560-image batch and
    autograd keeps ~30 MB per image-pass (~230 GB; the container has 64 GB) -- so the fixture is the oracle, which tests/
    test_oracle_golden.py pins to the reference's functions at every size that does fit, run here on the GPU box's host
    (3 TB, 256 cores; ~1-2 minutes at 32 threads).  Skipped when the host has less than 256 GB available."""
    if _C5:
        return _C5
    avail = 0
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable"):
            avail = int(line.split()[1]) // (1 << 20)
    if avail < 256:
        pytest.skip(f"config-5 oracle needs ~150 GB of host memory, {avail} GB available")
    import os
    from collections import OrderedDict
    from oracle import model as OM, steps as S
    hw, b, mu = 256, 128, 7
    nx, nu = 2 * b * 3, 2 * b * mu
    x, u_w, u_s = C.u8(9100, (nx, 3, hw, hw)), C.u8(9101, (nu, 3, hw, hw)), C.u8(9102, (nu, 3, hw, hw))
    y = C.ints(9103, (nx,), 2)

    def state():
        p, bufs = OM.split_state(OM.init_state(C.PARAM_SEED, OM.net_param_specs(), random_running_stats=True))
        pc, _ = OM.split_state(OM.init_state(C.PARAM_SEED + 1, OM.classifier_param_specs("finetune", 2)))
        p = OrderedDict(p)
        p.update(pc)
        return p, bufs
    ps, bs = state()
    pt, bt = state()
    for v in ps.values():
        v.requires_grad_(True)

    class KeepGrads:                       # an "optimizer" that only lets the step run its backward
        def zero_grad(self):
            pass

        def step(self):
            pass
    threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    try:
        o = S.ssl_cr_step("ce", ps, bs, pt, bt, KeepGrads(), x.float(), y, u_w.float(), u_s.float(), 1.0, faithful=False)
    finally:
        torch.set_num_threads(threads)
    names = list(ps.keys())
    _C5.update(x=x, y=y, u_w=u_w, u_s=u_s, loss=(o["loss"], o["loss_x"], o["loss_u"]), acc=o["acc"],
               logits=torch.cat((o["logits_x"], o["logits_u_s"])).double(), logits_t=o["logits_u_w"].double(),
               grads={k: ps[k].grad.double() for k in ("fc.0.weight", "classifier.0.weight", "model.layer4.1.conv2.weight",
                                                       "model.layer2.0.conv1.weight")},
               index={k: names.index(k) for k in names})
    return _C5


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_config5_per_gpu_shape_vs_oracle(dtype):
    """BASELINE config 5 (eval_Camelyon_SSL_CR.py:94-121 at --batch_size 1024 over 8 GPUs) at its own per-GPU shape, in the bf16
    engine mode and in the fp8 mode (e4m3 forward convs of layers 2-4), against the CPU oracle's iteration on the same inputs:
    losses, student / teacher logits, pseudo-label flips, and the gradients of four parameters from the head down to layer2.
    Bounds = 2 x the deviations measured on the MI355X (tests/measured_errors.json); the constants are ceilings."""
    from test_engine_gpu import build, freeze
    from ssl_cr_histo_amd import engine as E
    g = _config5_oracle()
    x, y, u_w, u_s = (g[k].to(DEV) for k in ("x", "y", "u_w", "u_s"))
    eng = E.Engine(DEV, dtype)
    mt, ct = build("finetune", "finetune", 2, True)
    ms, cs = build("finetune", "finetune", 2, True)
    state0 = {k: v.clone() for k, v in ms.state_dict().items()}
    freeze(mt, 64)
    mt.eval(); ms.train()
    te, st = eng.bind(mt, ct), eng.bind(ms, cs)
    if dtype == "fp8":          # delayed scaling: the first forward calibrates; undo its running-statistics update
        eng.step_ssl_cr(te, st, "ce", x, y, u_w, u_s, 1.0, backward=False)
        ms.load_state_dict(state0)
    r = eng.step_ssl_cr(te, st, "ce", x, y, u_w, u_s, 1.0)
    torch.cuda.synchronize()
    got = r["losses"].cpu().double()
    tag = f"config5_oracle/{dtype}"
    for i, nm in enumerate(("loss", "loss_x", "loss_u")):
        held(f"{tag}/{nm}", abs(float(got[i]) - g["loss"][i]) / abs(g["loss"][i]), 6e-2, floor=1e-3)
    lg, lt = r["logits"].cpu().double(), r["logits_t"].cpu().double()
    held(f"{tag}/logits", float((lg - g["logits"]).norm() / g["logits"].norm()), 0.3, floor=1e-2)
    held(f"{tag}/logits_t", float((lt - g["logits_t"]).norm() / g["logits_t"].norm()), 0.3, floor=1e-2)
    flips = int((lt.argmax(1) != g["logits_t"].argmax(1)).sum())
    assert flips <= max(2, lt.shape[0] // 200), flips
    assert abs(float(got[3]) / x.shape[0] - g["acc"]) <= 3.0 / x.shape[0]
    for k, want in g["grads"].items():
        mine = st.grad(g["index"][k]).cpu().double()
        held(f"{tag}/grad/{k}", float((mine - want).norm() / want.norm()), 0.9, floor=2e-2)
    del eng, te, st
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------ float64 per-element bounds
# tests/fp8_cases.py through kernels.conv2d_fp8: operands tests/_fp8.py, reference and bounds tests/_f64.py (fp8 section).
import math  # noqa: E402

import _f64 as B  # noqa: E402
import _fp8 as F8  # noqa: E402
from fp8_cases import CASES as F8_CASES  # noqa: E402

ROW_A, ROW_B, ROW_G = (1, 16, 16, 128, 128), (3, 32, 48, 128, 256), (4, 8, 8, 512, 512)
TRAIN_SET = "in_scale relu_in stats"
_F8_DEV = {}      # shape -> the operands on the device and the device's weight pack (one shape at a time)


def _f8_id(r):
    return f"{'x'.join('cus' if v is None else str(v) for v in r[0])}-{r[1].replace(' ', '+') or 'plain'}-xs{r[2]:g}"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _same_e4m3(w8, wq):
    """device codes [K, 3, 3, C] against float64 e4m3 values, bit for bit (the sign of zero included)"""
    got = w8.view(torch.float8_e4m3fn).float().cpu().double()
    return torch.equal(got, wq) and torch.equal(torch.signbit(got), torch.signbit(wq))


def _f8_operands(shape):
    from ssl_cr_histo_amd import kernels as K
    if shape not in _F8_DEV:
        _F8_DEV.clear()
        t = F8.inputs(shape)
        w8, dq, _ = K.pack_conv_fp8(t["w"].to(DEV))
        wq, dq_ref, _ = B.fp8_pack_ref(t["w"])
        assert _same_e4m3(w8, wq) and torch.equal(dq.cpu().double(), dq_ref)          # the launch and the reference use the same filters
        assert len(set(dq_ref.tolist())) >= 13 and float(dq_ref[3]) == 1.0
        d = dict(x=t["x"].to(DEV).to(torch.bfloat16), w8=w8, dq=dq, in_scale=t["in_scale"].to(DEV), in_shift=t["in_shift"].to(DEV),
                 bias=t["bias"].to(DEV), residual=t["residual"].to(DEV).to(torch.bfloat16))
        _F8_DEV[shape] = (t, d)
    return _F8_DEV[shape]


def _f8_launch(d, flags, xs, **extra):
    """-> (y, stats | None): y pre-filled with NaN (the wrapper pre-fills the statistics rows)"""
    from ssl_cr_histo_amd import kernels as K
    f = F8.flags_of(flags)
    kw = dict(extra)
    if "in_scale" in f:
        kw.update(in_scale=d["in_scale"], in_shift=d["in_shift"], in_relu="relu_in" in f)
    if "bias" in f:
        kw["bias"] = d["bias"]
    if "residual" in f:
        kw["residual"] = d["residual"]
    N, H, W, _ = d["x"].shape
    y = torch.full((N, H, W, d["w8"].shape[0]), float("nan"), dtype=torch.bfloat16, device=DEV)
    out = K.conv2d_fp8(d["x"], d["w8"], d["dq"], x_scale=xs, relu="relu" in f, want_stats="stats" in f, out=y, **kw)
    return out if "stats" in f else (out, None)


@pytest.mark.parametrize("row", F8_CASES, ids=[_f8_id(r) for r in F8_CASES])
def test_conv_fp8_f64(row):
    """every row of tests/fp8_cases.py: the launch is EXACTLY the row's instance, and y and the BatchNorm partial statistics hold the
    float64 per-element bounds of tests/_f64.py with the operands quantised as the kernel quantises them: bound() plus the measured
    alignment term of the fp8 MFMA (FP8_MFMA_U; the figure each row needs is printed).  No element is excused."""
    from ssl_cr_histo_amd import kernels as K
    shape, flags, xs, name, _ = row
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    walks = shape[0] is None
    shape = F8.batch(shape, cus)
    assert (F8.tiles(shape) > F8.walkers(shape, cus)) == walks, (shape, cus)
    t, d = _f8_operands(shape)
    y, stats = _f8_launch(d, flags, xs)
    assert K.last_conv_kernel == name, K.last_conv_kernel
    r = F8.reference(shape, flags, xs, t)
    what = f"fp8 {'x'.join(map(str, shape))} [{flags}] xs {xs:g}"
    print(f"[f64] {what} | {name} | over bound() without the alignment term: {B.fp8_align_needed(y, r['y'], r['mag'], r['pmax'], r['n']):.1f} u * pmax "
          f"(FP8_MFMA_MEASURED_U = {B.FP8_MFMA_MEASURED_U:g})")
    B.check(y, r["y"], r["bnd"], what, name)
    if stats is not None:
        assert stats.shape[0] == 4 * F8.tiles(shape)
        B.check_stats(stats, r["acc"], r["amag"], r["n"], what + " statistics", name, extra=B.fp8_align(r["pmax"]))


@pytest.mark.parametrize("flags", [TRAIN_SET, "bias residual relu"], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [ROW_A, ROW_G], ids=["a", "g"])
def test_conv_fp8_x_scale_dev(shape, flags):
    """x_scale_dev -- the only form the engine uses -- is read INSTEAD of the host x_scale: host 1.0 with a device 8.0 gives the bits of
    host 8.0, and not those of host 1.0"""
    _, d = _f8_operands(shape)
    dev8 = torch.full((1,), 8.0, device=DEV)
    y_dev, st_dev = _f8_launch(d, flags, 1.0, x_scale_dev=dev8)
    y_8, st_8 = _f8_launch(d, flags, 8.0)
    y_1, _ = _f8_launch(d, flags, 1.0)
    assert torch.isfinite(y_8.float()).all()
    assert torch.equal(_bits(y_dev), _bits(y_8))
    if st_8 is not None:
        assert torch.equal(_bits(st_dev), _bits(st_8))
    assert not torch.equal(_bits(y_dev), _bits(y_1))
    assert float(dev8) == 8.0


@pytest.mark.parametrize("flags, xs", [(TRAIN_SET, 1.0), ("in_scale stats", 3.0), ("", 16.0)], ids=["relu", "no_relu-xs3", "plain-xs16"])
@pytest.mark.parametrize("shape", [ROW_A, ROW_B, ROW_G], ids=["a", "b", "g"])
def test_conv_fp8_amax(shape, flags, xs):
    """amax_out, from 0: within one fp32 ulp of the reference's interval [max |relu(v)| / xs, max |v| / xs] (v the transformed activation
    before saturation: wide with the ReLU -- channel 0's in_scale is about -1e3 on a pixel of 1000 -- and a point without); a second
    launch into an amax_out holding twice that value leaves it bit-unchanged (the atomic only raises)"""
    t, d = _f8_operands(shape)
    f = F8.flags_of(flags)
    xf = dict(in_scale=t["in_scale"], in_shift=t["in_shift"], in_relu="relu_in" in f) if "in_scale" in f else {}
    _, (hi, lo) = B.fp8_activations(t["x"], xs, **xf)
    assert (lo < hi / 2) if "relu_in" in f else (lo == hi)
    amax = torch.zeros(1, device=DEV)
    _f8_launch(d, flags, xs, amax_out=amax)
    got = float(amax)
    print(f"[f64] amax {'x'.join(map(str, shape))} [{flags}] xs {xs:g}: got {got!r}, interval [{lo!r}, {hi!r}]")
    assert lo - F8.ulp32(lo) <= got <= hi + F8.ulp32(hi), (got, lo, hi)
    twice = torch.full((1,), 2.0 * got, device=DEV)
    _f8_launch(d, flags, xs, amax_out=twice)
    assert torch.equal(_bits(twice), _bits(torch.full((1,), 2.0 * got, device=DEV)))


def _planted_filters(Ko, Cc, seed):
    """filters whose per-channel amax sits on the frexp edge of the scale rule and at the ends of the range"""
    w = rnd(seed, (Ko, Cc, 3, 3), 0.05)
    edge = np.float32(448.0 * 2.0 ** -15)
    plant = {0: edge, 1: np.nextafter(edge, np.float32(0)), 2: np.nextafter(edge, np.float32(1)), 3: np.float32(1e-30), 4: np.float32(1e30)}
    for k, v in plant.items():
        i = int(w[k].abs().argmax())
        w[k] = (w[k].double() * (float(v) / float(w[k].abs().max()))).float()
        w[k].view(-1)[i] = float(v) * (1.0 if i % 2 else -1.0)
        assert float(w[k].abs().max()) == float(v)
    w[5] = 0.0
    w[6] *= 37.0
    w[7] *= 1e-3
    return w, plant


@pytest.mark.parametrize("Ko, Cc", [(16, 128), (9, 384)])
def test_pack_fp8_f64(Ko, Cc):
    """pack_fp8_kernel against the float64 restatement: without the BatchNorm fold every code and every dequant bit for bit, with amax
    planted on the frexp edge 448 * 2^-15, its two fp32 neighbours, 1e-30, 1e30 and 0; with the fold (one fp32 ulp of w * f can flip an
    e4m3 rounding) at most 1e-4 of the codes differ, and a gamma = 0 channel packs to zeros with dequant 1 and bias beta"""
    from ssl_cr_histo_amd import kernels as K
    w, plant = _planted_filters(Ko, Cc, 41)
    w8, dq, _ = K.pack_conv_fp8(w.to(DEV))
    wq, dq_ref, _ = B.fp8_pack_ref(w)
    assert torch.equal(dq.cpu().double(), dq_ref), (dq.cpu(), dq_ref)
    assert _same_e4m3(w8, wq)
    assert [float(v) for v in dq_ref[:6]] == [2.0 ** -15, 2.0 ** -15, 2.0 ** -14, 2.0 ** -108, 2.0 ** 91, 1.0]
    top = wq.abs().flatten(1).max(1).values
    assert float(top[0]) == 448.0 and float(top[5]) == 0.0 and bool(((top >= 224.0) & (top <= 448.0))[[1, 2, 3, 4, 6, 7, 8]].all())
    # the fold
    w = rnd(42, (Ko, Cc, 3, 3), 0.05)
    gamma, beta, rmean, rvar = rnd(43, (Ko,)).abs() + 0.5, rnd(44, (Ko,)), rnd(45, (Ko,)), rnd(46, (Ko,)).abs() + 0.5
    gamma[7] = 0.0
    bn = (gamma, beta, rmean, rvar)
    w8f, dqf, bias = K.pack_conv_fp8(w.to(DEV), bn=tuple(v.to(DEV) for v in bn))
    wqf, dqf_ref, bias_ref = B.fp8_pack_ref(w, bn=bn)
    assert torch.equal(dqf.cpu().double(), dqf_ref)
    gotf = w8f.view(torch.float8_e4m3fn).float().cpu().double()
    flipped = float((gotf != wqf).double().mean())
    print(f"[f64] pack_fp8 with the fold, K {Ko} C {Cc}: share of flipped codes {flipped:.2e}")
    assert flipped < 1e-4
    assert float(gotf[7].abs().max()) == 0.0 and float(dqf[7]) == 1.0 and float(bias[7]) == float(beta[7])
    f = gamma.double() / torch.sqrt(rvar.double() + 1e-5)
    B.check(bias, bias_ref, 2 * B.U * (beta.double().abs() + (rmean.double() * f).abs()) + 4 * B.U * (rmean.double() * f).abs(), "folded bias", dims="k")


def test_fp8_scale_update():
    """fp8_scale_update_kernel through sslcr_fp8_scale_update: n = 70 slots (two 64-thread blocks, the second ragged) inside a buffer
    of 80; scale <- clamp(2^floor(log2(224 / amax)), 2^-16, 2^16) where 0 < amax < 3e38, else unchanged; every amax word 0 afterwards;
    slots beyond n untouched.  (Values within 2 fp32 ulps of 224 * 2^k other than the exact ones are left out: there the fp32 quotient
    may round across the power of two.)"""
    from ssl_cr_histo_amd import kernels as K
    vals = [0.0, -1.0, float("nan"), float("inf"), 3.2e38, 1e-30, 1e30, 224.0, 448.0, 28.0, 7168.0, 100.0, 0.01, 223.0, 225.0]
    want = [None, None, None, None, None, 65536.0, 2.0 ** -16, 1.0, 0.5, 8.0, 2.0 ** -5, 2.0, 16384.0, 1.0, 0.5]
    n, total = 70, 80
    slots = torch.empty((total, 2), dtype=torch.float32)
    slots[:, 0] = torch.arange(total, dtype=torch.float32) + 3.0
    slots[:, 1] = torch.tensor([vals[i % len(vals)] for i in range(total)])
    dev = slots.to(DEV)
    K.fp8_scale_update(dev[:n])
    got = dev.cpu()
    expect = slots.clone()
    for i in range(n):
        m = vals[i % len(vals)]
        if want[i % len(vals)] is not None:
            s = min(max(2.0 ** math.floor(math.log2(224.0 / m)), 2.0 ** -16), 2.0 ** 16)
            assert s == want[i % len(vals)], (m, s)
            expect[i, 0] = s
        expect[i, 1] = 0.0
    assert torch.equal(expect[:n], B.fp8_scale_update_ref(slots[:n]))          # the float64 restatement agrees with the literal table
    assert torch.equal(_bits(got[:n, 1]), torch.zeros(n, dtype=torch.int32))   # +0.0, the NaN and the negative entries included
    assert torch.equal(_bits(got[:n, 0]), _bits(expect[:n, 0])), (got[:n, 0], expect[:n, 0])
    assert torch.equal(_bits(got[n:]), _bits(slots[n:]))                       # (NaN bits compared as integers)


@pytest.mark.parametrize("flags, xs", [("", 1.0), (TRAIN_SET, 1.0), ("in_scale stats", 1.0), (TRAIN_SET, 0.25), (TRAIN_SET, 16.0), ("", 16.0)],
                         ids=["plain", "train", "no_relu", "train-xs0.25", "train-xs16", "plain-xs16"])
@pytest.mark.parametrize("shape", [ROW_A, (2, 16, 16, 512, 512), ROW_G], ids=["a", "four_slabs", "g"])
def test_conv_fp8_load_path_quantiser_is_exact(shape, flags, xs):
    """the load path alone, bit for bit: with identity centre-tap filters (K = C; every weight scale 2^8) an output element is ONE
    non-zero product, xq * 256 * 2^-8 / xs -- exact in fp32 and in bf16 for a power-of-two x_scale -- so y must EQUAL the reference's
    e4m3 activations / xs: the tie rule, the subnormals, the saturation, in_scale * xs per channel of every slab, the ReLU clamp, and
    the zero pixel.  (This is the check the alignment term of the bound cannot blur.)"""
    from ssl_cr_histo_amd import kernels as K
    N, H, W, Cc, Ko = shape
    assert Cc == Ko
    t = F8.inputs(shape)
    w = torch.zeros((Ko, Cc, 3, 3))
    w[torch.arange(Ko), torch.arange(Cc), 1, 1] = 1.0
    w8, dq, _ = K.pack_conv_fp8(w.to(DEV))
    assert set(dq.cpu().tolist()) == {2.0 ** -8}
    f = F8.flags_of(flags)
    xf = dict(in_scale=t["in_scale"], in_shift=t["in_shift"], in_relu="relu_in" in f) if "in_scale" in f else {}
    y = torch.full((N, H, W, Ko), float("nan"), dtype=torch.bfloat16, device=DEV)
    K.conv2d_fp8(t["x"].to(DEV).to(torch.bfloat16), w8, dq, x_scale=xs, out=y, **{k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in xf.items()})
    xq, _ = B.fp8_activations(t["x"], xs, **xf)
    want = xq / xs
    got = y.float().cpu().double()
    bad = (got != want).nonzero()
    assert bad.shape[0] == 0, (f"{bad.shape[0]} of {got.numel()} activations quantised differently, first at (n, h, w, c) = {bad[0].tolist()}: "
                               f"got {float(got[tuple(bad[0])])!r} want {float(want[tuple(bad[0])])!r}")
    if xs == 1.0 and not f:
        assert int((xq[..., F8.SUB].abs() < 2.0 ** -6).sum()) > 0.9 * xq[..., F8.SUB].numel()        # the subnormal channel is one
        assert float(xq[0, 0, 0, :8].min()) == 448.0 and float(xq[N - 1, H // 2, W // 2].abs().max()) == 0.0

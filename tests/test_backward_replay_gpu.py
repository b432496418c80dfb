"""Layer-wise backward replay at FULL size: every weight-gradient and data-gradient kernel launch of one SSL_CR step at the
benchmark's shape (student 192 + 448 = 640 images of 256x256) is checked on the tensors the engine itself fed it.

The engine-level gradient tests compare final gradients with the reference's, where bf16 storage of the *forward* alone moves the
early layers by tens of percent -- a bound that cannot see a 10 % error in one backward kernel.  Here the debug tap
(include/sslcr.h: sslcr_net_debug_tap / sslcr_net_debug_tensor) hands back, per BasicBlock, the saved activations X and the
transient gradients dY exactly as the kernels read them; the oracle (oracle/kernels_ref.py: torch-CPU fp32 autograd formulas of
nn.Conv2d, the ops torchvision resnet18 runs under models/net.py:32,77) recomputes dW and dX from those same tensors, so what is
left is the kernel's own arithmetic: 1.2e-2 of the tensor's max in bf16 (output rounding), 2e-4 in fp32 -- the per-kernel bounds of
tests/test_kernels_gpu.py, now at 640 x 64^2 ... 640 x 8^2 instead of <= 72 images of <= 32 x 32.

The second half of the file (test_step_replay_f64 and what follows) replays EVERY pass and stage of a step -- forward, BatchNorm
statistics, backward, parameter gradients -- in float64 with the per-element bounds of tests/_f64.py, at small shapes chosen so that
every form the engine can give a block is taken by some row; tests/test_step_replay_cpu.py runs the same checks on an emulated step."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cases as C  # noqa: E402
from oracle import kernels_ref as R  # noqa: E402

from test_engine_gpu import _engine, build, freeze  # noqa: E402
from test_kernels_gpu import close  # noqa: E402

TOL = {"fp32": 2e-4, "bf16": 1.2e-2}
BLOCKS = [f"layer{l}.{b}" for l in (1, 2, 3, 4) for b in (0, 1)]


def _q(t, dtype):
    return t.to(torch.bfloat16).float() if dtype == "bf16" else t.float()


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_every_backward_conv_kernel_on_the_engines_own_tensors(dtype):
    eng = _engine(dtype)
    name = "bpq_cr_full"
    c = C.CASES[name]
    mt, ct = build("finetune", "finetune", 1, True)
    ms, cs = build("finetune", "finetune", 1, True)
    freeze(mt, 64)
    freeze(ms, 0)
    (xl, yl), = C.labeled_batches(name)
    (uw, us), = C.unlabeled_batches(name)
    te, st = eng.bind(mt, ct), eng.bind(ms, cs)
    mt.eval()
    ms.train()
    hw = c["hw"]
    st.debug_tap(True)
    try:
        eng.step_ssl_cr(te, st, "mse", xl.reshape(-1, 3, hw, hw), yl.reshape(-1), uw, us, c["lambda_u"])
        torch.cuda.synchronize()
        pnames = [k for k, _ in ms.named_parameters()]
        params = dict(ms.named_parameters())
        threads = torch.get_num_threads()
        torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))     # torch-CPU convolutions get slower beyond ~32 threads
        report = []
        try:
            for blk in range(7, -1, -1):
                pre = f"model.{BLOCKS[blk]}"
                has_ds = f"{pre}.downsample.0.weight" in params
                stride = 2 if has_ds else 1

                def T(kind):
                    t, fl = st.debug_tensor(blk, kind)
                    return t.float().cpu(), fl

                def grad_krsc(pname):
                    return st.grad(pnames.index(pname)).cpu().permute(0, 2, 3, 1).contiguous()

                def w_krsc(pname):
                    return _q(params[pname].detach().cpu(), dtype).permute(0, 2, 3, 1).contiguous()
                x_in, _ = T(10)
                raw1, _ = T(6)
                sc1, sh1 = T(11)[0], T(12)[0]
                G, _ = T(0)
                dRaw2, _ = T(1)
                dAct1, flags = T(2)
                dRaw1, _ = T(3)
                N, oh, ow, K = dRaw2.shape
                xh, xw = x_in.shape[1], x_in.shape[2]
                # ---- conv2: wgrad on relu(bn1(raw1)) computed on the fly, dgrad (+ bn1's ReLU mask where the kernel fuses it)
                pre1 = raw1.double() * sc1.double() + sh1.double()
                x2 = _q(torch.clamp_min(raw1 * sc1 + sh1, 0.0), dtype)
                close(grad_krsc(f"{pre}.conv2.weight"), R.conv_wgrad(x2, dRaw2, (K, 3, 3, K), 1, 1), TOL[dtype], f"{pre}.conv2 wgrad")
                want = R.conv_dgrad(dRaw2, w_krsc(f"{pre}.conv2.weight"), 1, 1, (oh, ow))
                if flags & 1:
                    # the mask is a sign decision on an fp32 fma: leave out the elements whose pre-activation is zero to rounding
                    tie = pre1.abs() <= 1e-6 * (raw1.double() * sc1.double()).abs().clamp_min(1e-30)
                    want = torch.where(pre1 > 0, want, torch.zeros_like(want))
                    want = torch.where(tie, dAct1, want)
                close(dAct1, want, TOL[dtype], f"{pre}.conv2 dgrad (mask fused: {flags & 1})")
                del pre1, x2, want, dAct1, raw1
                # ---- conv1 (3x3, stride 1 or 2) and the 1x1/2 projection: wgrads, and the block-input gradient they sum to
                C1 = x_in.shape[3]
                close(grad_krsc(f"{pre}.conv1.weight"), R.conv_wgrad(x_in, dRaw1, (K, 3, 3, C1), stride, 1), TOL[dtype], f"{pre}.conv1 wgrad")
                want = R.conv_dgrad(dRaw1, w_krsc(f"{pre}.conv1.weight"), stride, 1, (xh, xw))
                if has_ds:
                    dRawD, _ = T(4)
                    close(grad_krsc(f"{pre}.downsample.0.weight"), R.conv_wgrad(x_in, dRawD, (K, 1, 1, C1), 2, 0), TOL[dtype],
                          f"{pre}.downsample.0 wgrad")
                    want = want + R.conv_dgrad(dRawD, w_krsc(f"{pre}.downsample.0.weight"), 2, 0, (xh, xw))
                else:
                    want = want + G
                dXin, _ = T(5)
                close(dXin, want, TOL[dtype], f"{pre} block-input gradient (conv1 dgrad + shortcut)")
                report.append(f"{pre}: N={N} {xh}x{xw}x{C1} -> {oh}x{ow}x{K} ok")
        finally:
            torch.set_num_threads(threads)
        print(f"[{dtype}] backward replay:\n   " + "\n   ".join(report))
    finally:
        st.debug_tap(False)


# ====================================================================================================================
# The float64 replay of every pass and stage of one engine step.
#
# The test above holds the conv gradients of a single-branch step to 1.2e-2 / 2e-4 of the tensor maximum.  Here every stage of every
# block -- forward and backward, every pass of a TripletNet -- is recomputed in float64 from the tensors the engine itself fed that
# stage (sslcr_net_debug_tensor, kind | pass << 8) and held to the per-element bound tests/_f64.py derives for the operation, through
# the descriptors csrc/engine.cpp builds: segments or pass by pass, which saved statistics, which count, which scratch slot.
# The rows and the form word each (row, block) must report: tests/step_forms.py (computed on the CPU, tests/test_kernel_routes_cpu.py).
#
# Bounds that chain two kernels are put together from the single-kernel bounds as follows (u_out = 2^-8 for bf16 storage, else 0):
#   saved statistics   the conv's statistics rows are not kept: B.stats_bound gives the error of their two sums against the float64
#                      accumulator, B.bn_finalize_ref carries it through mean / var / invstd / scale / shift and the running statistics
#                      (its chained form, see there).
#   BatchNorm backward the reduce pass's sums are not kept either: B.bn_bwd_sums_ref gives them (s) and their bound (sb); dx = sc g + cB x
#                      - sc s0/n - cB mean with cB = -sc is^2 s1/n moves by at most  |sc| sb0 / n + |sc| is^2 |x - mean| sb1 / n  (times 1 +
#                      u_out), added to B.bn_bwd_apply_ref's bound; dgamma, dbeta by  sum_p sb1 is  and  sum_p sb0.
#   fused bn1 mask     the dgrad leaves bn1's sums from its fp32 ACCUMULATOR under the mask: the sums of the float64 dgrad under the
#                      float64 mask, each term carrying the accumulator's bound e (B.bound(..., out_dtype 0)): sb0 += sum e, sb1 += sum
#                      e |x - mean|; an element within B.mask_unsure's band may be on either side: sb += its whole term.
#   projection block   dXin is written twice: the 3x3 / 2 input gradient d3 (stored: error pb3 = B.parity_bound), then the 1x1 / 2 scatter
#                      adds d1 to the STORED value at the even positions: there  pb3 + u_out pb3 + B.bound(d3 + d1, mag1 + |d3| + pb3, K),
#                      elsewhere pb3.
# ====================================================================================================================
import _f64 as B  # noqa: E402
import step_forms as SF  # noqa: E402

ROW_ORDER = list(SF.ROWS)
MULTI_PASS = [k for k in ROW_ORDER if SF.ROWS[k][1]]          # the TripletNet rows, first in ROW_ORDER: A, B, C
NAMES = ("conv1", "bn1", "conv2", "bn2", "downsample.0", "downsample.1")


def _run_row(key, tap=True):
    """one step of row `key` from fresh modules -> (bound net, modules, loss, running statistics before the step)"""
    dtype, triplet, N, hw = SF.ROWS[key]
    eng = _engine(dtype)
    if triplet:
        model, cls = build("triplet", "mlp", 6, False)
        model.train()
        cls.train()
        net = eng.bind(model, cls)
        xs = [C.u8(9100 + i, (N, 3, hw, hw)) for i in range(3)]
        y = C.ints(9104, (N,), 6).long()
    else:
        mt, ct = build("finetune", "finetune", 2, True)
        model, cls = build("finetune", "finetune", 2, True)
        mt.eval()
        ct.eval()
        model.train()
        cls.train()
        te, net = eng.bind(mt, ct), eng.bind(model, cls)
        nx = N // 4
        x, uw, us = C.u8(9110, (nx, 3, hw, hw)), C.u8(9111, (N - nx, 3, hw, hw)), C.u8(9112, (N - nx, 3, hw, hw))
        y = C.ints(9113, (nx,), 2).long()
    before = {k: v.detach().clone().cpu() for k, v in model.state_dict().items() if "running_" in k}
    net.debug_tap(tap)
    if triplet:
        r = eng.step_supervised(net, "ce", xs, y, train=True)
    else:
        r = eng.step_ssl_cr(te, net, "ce", x, y, uw, us, 1.0)
    torch.cuda.synchronize()
    return net, model, cls, r["losses"].cpu(), before


@pytest.fixture(scope="module", params=ROW_ORDER)
def step(request):
    """everything one step of the row left, on the host in the storage dtype: blocks[i][p][name], weights, gradients, statistics"""
    key = request.param
    dtype, triplet, N, hw = SF.ROWS[key]
    net, model, cls, losses, before = _run_row(key)
    npass = 3 if triplet else 1
    try:
        pnames = [k for k, _ in model.named_parameters()]
        params = {k: v.detach().cpu() for k, v in model.named_parameters()}
        grads = {k: net.grad(i).cpu() for i, k in enumerate(pnames)}
        after = {k: v.detach().clone().cpu() for k, v in model.state_dict().items() if "running_" in k}
        blocks, forms, packs = [], [], []
        kinds = dict(G=0, dRaw2=1, dAct1=2, dRaw1=3, dXin=5, raw1=6, raw2=7, y=9, x=10, dOut=29)
        vecs = dict(bn1=11, bn2=21, bnd=25)
        for i in range(8):
            has_ds = SF.BLOCK_CFG[i][2] == 2
            per = []
            for p in range(npass):
                d = {}
                for name, k in kinds.items():
                    d[name], fl = net.debug_tensor(i, k, p)
                    d[name] = d[name].cpu()
                if has_ds:
                    d["dRawD"], d["rawd"] = net.debug_tensor(i, 4, p)[0].cpu(), net.debug_tensor(i, 8, p)[0].cpu()
                for name, k in vecs.items():
                    if name != "bnd" or has_ds:       # -> (scale, shift, mean, invstd)
                        d[name] = tuple(net.debug_tensor(i, k + j, p)[0].cpu() for j in range(4))
                per.append(d)
            blocks.append(per)
            forms.append(fl)
            packs.append({c: net.debug_tensor(i, k)[0].float().cpu() for c, k in (("conv1", 15), ("conv2", 17)) + ((("ds", 19),) if has_ds else ())})
        segs = bool(net.segments_used)
    finally:
        net.debug_tap(False)
    torch.cuda.synchronize()
    return dict(key=key, dt=1 if dtype == "bf16" else 0, npass=npass, N=N, blocks=blocks, forms=forms, packs=packs, params=params,
                grads=grads, before=before, after=after, segs=segs, losses=losses, ratios={})


def _worst(got, want, bnd, skip=None):
    r = B.ratio(got, want, bnd)
    if skip is not None:
        r = torch.where(skip, torch.zeros_like(r), r)
    return float(r.max())


class _Block:
    """the float64 references of one block of one row, stage by stage.  Every method returns (got, want, bound[, skip]) for B.check, from
    the tensors the engine fed the stage; `stats` / `count_mul` let the sensitivity test feed a stage another pass's statistics"""

    def __init__(self, s, i):
        self.s, self.i = s, i
        self.dt, self.f32, self.npass, self.N = s["dt"], s["dt"] == 0, s["npass"], s["N"]
        self.cin, self.cout, self.stride = SF.BLOCK_CFG[i]
        self.has_ds = self.stride == 2
        self.P = s["blocks"][i]
        self.W = s["packs"][i]
        self.word = s["forms"][i]
        self.oh, self.ow = self.P[0]["raw1"].shape[1:3]
        self.xh, self.xw = self.P[0]["x"].shape[1:3]
        self.count = self.N * self.oh * self.ow
        self.pre = "model.layer%d.%d." % (i // 2 + 1, i % 2)
        self._cache = {}

    def memo(self, key, fn):
        if key not in self._cache:
            self._cache[key] = fn()
        return self._cache[key]

    # ---- forward
    def conv1(self, p):
        d = self.P[p]
        return self.memo(("c1", p), lambda: B.conv_fwd(d["x"], self.W["conv1"], self.stride, 1))

    def act1(self, p, stats=None):
        sc, sh = self.P[p if stats is None else stats]["bn1"][:2]
        return B.xform(self.P[p]["raw1"], sc, sh, True, self.dt)

    def conv2(self, p, stats=None):
        return self.memo(("c2", p, stats), lambda: B.conv_fwd(self.act1(p, stats), self.W["conv2"], 1, 1))

    def convd(self, p):
        return self.memo(("cd", p), lambda: B.conv_fwd(self.P[p]["x"], self.W["ds"], 2, 0))

    def raw(self, which, p, stats=None):
        want, mag, _, _ = {"raw1": self.conv1, "rawd": self.convd}[which](p) if which != "raw2" else self.conv2(p, stats)
        n = {"raw1": 9 * self.cin, "raw2": 9 * self.cout, "rawd": self.cin}[which]
        return self.P[p][which], want, B.bound(want, mag, n, self.dt, self.f32)

    def saved(self, bn):
        """-> B.bn_finalize_ref of BatchNorm `bn` over all passes in branch order, from the float64 accumulators"""
        which = {"bn1": "conv1", "bn2": "conv2", "bnd": "downsample.0"}[bn]
        n = {"bn1": 9 * self.cin, "bn2": 9 * self.cout, "bnd": self.cin}[bn]
        conv = {"bn1": self.conv1, "bn2": self.conv2, "bnd": self.convd}[bn]
        mod = {"bn1": "bn1", "bn2": "bn2", "bnd": "downsample.1"}[bn]
        sums, errs = [], []
        for p in range(self.npass):
            _, _, acc, amag = conv(p)
            s_, ss, bs, bss = B.stats_bound(acc, amag, n, self.f32)
            sums.append(torch.stack([s_, ss]))
            errs.append((bs, bss))
        from ssl_cr_histo_amd import _lib
        rows = SF.stats_rows(_lib.lib(), self.s["key"], self.i, self.word)[{"bn1": 0, "bn2": 1, "bnd": 2}[bn]]
        pr, st = self.s["params"], self.s["before"]
        return B.bn_finalize_ref(torch.stack(sums), float(self.count), pr[self.pre + mod + ".weight"], pr[self.pre + mod + ".bias"],
                                 st[self.pre + mod + ".running_mean"], st[self.pre + mod + ".running_var"],
                                 replay=1 if self.npass > 1 else 3, nseg=self.npass, rows=rows,
                                 sum_err=(torch.stack([e[0] for e in errs]), torch.stack([e[1] for e in errs]))), which

    def y(self, p):
        d = self.P[p]
        sc, sh = d["bn2"][:2]
        if self.has_ds:
            want, mag = B.bn_act_ref(d["raw2"], sc, sh, res=d["rawd"], rsc=d["bnd"][0], rsh=d["bnd"][1])
        else:
            want, mag = B.bn_act_ref(d["raw2"], sc, sh, res=d["x"])
        return d["y"], want, B.bound(want, mag, 0, self.dt)

    # ---- backward
    def bn_bwd(self, g64, gmag, x, bn, count, g_for_apply=None, e_g=None, unsure=None):
        """-> (dx64, bound, sums64 [2, C], their bound): the module text's chain.  bn = (scale, shift, mean, invstd)"""
        sc, _, mean, invstd = bn
        s, sb = B.bn_bwd_sums_ref(g64, gmag, x, mean)
        s, sb = s[0], sb[0]
        C_ = x.shape[-1]
        xm = (x.double() - mean.double()).abs()
        if e_g is not None:
            sb = sb + torch.stack([e_g.reshape(-1, C_).sum(0), (e_g * xm).reshape(-1, C_).sum(0)])
        if unsure is not None:
            t = torch.where(unsure, gmag + (e_g if e_g is not None else 0.0), torch.zeros_like(gmag))
            sb = sb + torch.stack([t.reshape(-1, C_).sum(0), (t * xm).reshape(-1, C_).sum(0)])
        ga = g64 if g_for_apply is None else g_for_apply
        dx, bnd = B.bn_bwd_apply_ref(ga, x, sc, invstd, mean, s, count, self.dt)
        u_out = B.U_BF16 if self.dt == 1 else 0.0
        scd, isd = sc.double().abs(), invstd.double()
        bnd = bnd + (1 + u_out) * (scd * sb[0] / count + scd * isd * isd * xm * sb[1] / count)
        return dx, bnd, s, sb

    def bn2_bwd(self, p, stats=None, count_mul=1):
        d = self.P[p]
        G = d["G"].double()
        q = self.P[p if stats is None else stats]
        out = {}
        dx, bnd, s, sb = self.bn_bwd(G, G.abs(), d["raw2"], q["bn2"], self.count * count_mul)
        out["dRaw2"] = (d["dRaw2"], dx, bnd, s, sb)
        if self.has_ds:
            dx, bnd, s, sb = self.bn_bwd(G, G.abs(), d["rawd"], q["bnd"], self.count * count_mul)
            out["dRawD"] = (d["dRawD"], dx, bnd, s, sb)
        return out

    def w_krsc(self, name):
        return self.W[name]

    def dact1(self, p):
        """-> (got, want, bound, skip, (g64, gmag, e_acc, unsure) for bn1)"""
        d = self.P[p]
        want, mag = B.conv_dgrad(d["dRaw2"], self.W["conv2"], 1, 1, (self.oh, self.ow))
        n = 9 * self.cout
        skip = None
        if self.word & SF.MASK:
            sc, sh = d["bn1"][:2]
            x = d["raw1"].double()
            pre, premag = x * sc.double() + sh.double(), x.abs() * sc.double().abs() + sh.double().abs()
            skip = B.mask_unsure(pre, premag)
            keep = pre > 0
            want, mag = torch.where(keep, want, torch.zeros_like(want)), torch.where(keep, mag, torch.zeros_like(mag))
        return d["dAct1"], want, B.bound(want, mag, n, self.dt, self.f32), skip, (want, mag, B.bound(want, mag, n, 0, self.f32), skip)

    def bn1_bwd(self, p):
        d = self.P[p]
        if self.word & SF.MASK:     # sums from the dgrad's accumulator under the mask; the apply pass reads the stored, masked dAct1
            _, _, _, _, (g64, gmag, e_acc, unsure) = self.memo(("da", p), lambda: self.dact1(p))
            dx, bnd, s, sb = self.bn_bwd(g64, gmag, d["raw1"], d["bn1"], self.count, g_for_apply=d["dAct1"].double(), e_g=e_acc, unsure=unsure)
        else:                       # relu_from_x: the sign of fmaf(x, scale, shift), exact in float64
            g64, gmag = B.bn_bwd_g(d["dAct1"], d["raw1"], d["bn1"][0], d["bn1"][1], relu_from_x=True)
            dx, bnd, s, sb = self.bn_bwd(g64, gmag, d["raw1"], d["bn1"], self.count)
        return d["dRaw1"], dx, bnd, s, sb

    def dxin(self, p):
        d = self.P[p]
        w1 = self.W["conv1"]
        if not self.has_ds:
            want, mag = B.conv_dgrad(d["dRaw1"], w1, 1, 1, (self.xh, self.xw), residual=d["G"])
            return d["dXin"], want, B.bound(want, mag, 9 * self.cout, self.dt, self.f32)
        d3, mag3 = B.conv_dgrad(d["dRaw1"], w1, 2, 1, (self.xh, self.xw))
        pb3 = B.parity_bound(d3, mag3, self.cout, self.dt, self.f32)
        d1, mag1 = B.conv_dgrad(d["dRawD"], self.W["ds"], 2, 0, (self.xh, self.xw))
        u_out = B.U_BF16 if self.dt == 1 else 0.0
        reach = B.scatter_reach(d3.shape).view(1, self.xh, self.xw, 1)
        both = pb3 + u_out * pb3 + B.bound(d3 + d1, mag1 + d3.abs() + pb3, self.cout, self.dt, self.f32)
        assert float(d1[:, ~reach[0, :, :, 0]].abs().max()) == 0.0
        return d["dXin"], d3 + d1, torch.where(reach, both, pb3)

    # ---- the gradients of the parameters, over all passes
    def wgrad(self, conv):
        xs, dys = [], []
        for p in range(self.npass):
            d = self.P[p]
            xs.append(self.act1(p) if conv == "conv2" else d["x"].double())
            dys.append(d[{"conv1": "dRaw1", "conv2": "dRaw2", "ds": "dRawD"}[conv]].double())
        x, dy = torch.cat(xs), torch.cat(dys)
        R_, st_, pad = {"conv1": (3, self.stride, 1), "conv2": (3, 1, 1), "ds": (1, 2, 0)}[conv]
        want, mag = B.conv_wgrad(x, dy, (self.cout, R_, R_, x.shape[-1]), st_, pad)
        pname = self.pre + {"conv1": "conv1", "conv2": "conv2", "ds": "downsample.0"}[conv] + ".weight"
        got = self.s["grads"][pname].permute(0, 2, 3, 1).contiguous()
        return got, want, B.bound(want, mag, self.npass * self.count, 0, self.f32)

    def bn_grads(self, bn, sums):
        """sums: per pass (s64 [2, C], bound) -> ((got dgamma, want, bound), (got dbeta, want, bound))"""
        mod = {"bn1": "bn1", "bn2": "bn2", "bnd": "downsample.1"}[bn]
        s = torch.stack([a for a, _ in sums])
        sb = torch.stack([b for _, b in sums])
        invstd = torch.stack([self.P[p][bn][3] for p in range(self.npass)])
        z = torch.zeros(s.shape[-1])
        wg, bg, wb, bb = B.bn_param_grads_ref(s, invstd, z, z)
        bg = bg + (sb[:, 1] * invstd.double()).sum(0)
        bb = bb + sb[:, 0].sum(0)
        return (self.s["grads"][self.pre + mod + ".weight"], wg, bg), (self.s["grads"][self.pre + mod + ".bias"], wb, bb)


@pytest.mark.parametrize("blk", range(8))
def test_step_replay_f64(step, blk):
    """every stage of block `blk`, every pass, within its float64 bound; the form word the engine reports is the CPU table's"""
    from ssl_cr_histo_amd import _lib
    key = step["key"]
    b = _Block(step, blk)
    want_word = SF.expected_forms(_lib.lib(), key)[blk]
    assert b.word == want_word, f"row {key} block {blk}: the engine reports {SF.word_str(b.word)}, the routing says {SF.word_str(want_word)}"
    assert step["segs"] == bool(b.word & SF.FWD_SEG)
    tag = f"row {key} block {blk}"
    worst = {}

    def chk(stage, got, want, bnd, skip=None, dims="nhwk"):
        if skip is not None:
            B.capped(skip, f"{tag} {stage}")
            want = torch.where(skip, got.double(), want)
        worst[stage] = max(worst.get(stage, 0.0), B.check(got, want, bnd, f"{tag} {stage}", SF.word_str(b.word), dims=dims))

    sums = {"bn1": [], "bn2": [], "bnd": []}
    for p in range(b.npass):
        d = b.P[p]
        # ---- forward
        chk("raw1", *b.raw("raw1", p))
        chk("raw2", *b.raw("raw2", p))
        if b.has_ds:
            chk("rawd", *b.raw("rawd", p))
        chk("y", *b.y(p))
        # ---- backward
        keep = d["y"].float() > 0
        assert torch.equal(d["G"].float(), torch.where(keep, d["dOut"].float(), torch.zeros(()))), f"{tag} pass {p}: G is dOut under (y > 0), bit for bit"
        for name, (got, want, bnd, s_, sb) in b.bn2_bwd(p).items():
            chk(name, got, want, bnd)
            sums["bn2" if name == "dRaw2" else "bnd"].append((s_, sb))
        got, want, bnd, skip, _ = b.memo(("da", p), lambda: b.dact1(p))
        chk("dAct1", got, want, bnd, skip)
        got, want, bnd, s_, sb = b.bn1_bwd(p)
        chk("dRaw1", got, want, bnd)
        sums["bn1"].append((s_, sb))
        chk("dXin", *b.dxin(p))
    # ---- the saved statistics of the three BatchNorms and their running statistics after the step, in branch order
    for bn in ("bn1", "bn2") + (("bnd",) if b.has_ds else ()):
        ref, _ = b.saved(bn)
        for j, name in enumerate(("scale", "shift", "mean", "invstd")):
            got = torch.stack([b.P[p][bn][j] for p in range(b.npass)])
            chk(f"{bn} {name}", got, ref[name][0], ref[name][1], dims="pc")
        mod = {"bn1": "bn1", "bn2": "bn2", "bnd": "downsample.1"}[bn]
        chk(f"{bn} running_mean", step["after"][b.pre + mod + ".running_mean"], *ref["running_mean"], dims="c")
        chk(f"{bn} running_var", step["after"][b.pre + mod + ".running_var"], *ref["running_var"], dims="c")
        (gg, wg, bg), (gb, wb, bb) = b.bn_grads(bn, sums[bn])
        chk(f"{bn} dgamma", gg, wg, bg, dims="c")
        chk(f"{bn} dbeta", gb, wb, bb, dims="c")
    # ---- weight gradients over ALL passes
    for conv in ("conv1", "conv2") + (("ds",) if b.has_ds else ()):
        chk(f"{conv} wgrad", *b.wgrad(conv), dims="krsc")
    print(f"[replay] {tag} forms {SF.word_str(b.word)} | " + " ".join(f"{k.replace(' ', '_')}={v:.4f}" for k, v in worst.items()))


@pytest.mark.parametrize("step", MULTI_PASS, indirect=True)
@pytest.mark.parametrize("blk", [0, 5])
def test_step_replay_sees_foreign_statistics_and_counts(step, blk):
    """the bounds are tight enough for the bugs they are there for: pass 1 checked against a reference built from pass 0's saved
    statistics, or with a count of 3 N oh ow, lies OVER its bound (multi-pass rows; elementwise on the host, nothing runs on the device)"""
    b = _Block(step, blk)
    got, want, bnd = b.raw("raw2", 1)
    assert _worst(got, want, bnd) <= 1.0
    got, want, bnd = b.raw("raw2", 1, stats=0)
    r_fwd = _worst(got, want, bnd)
    got, want, bnd, _, _ = b.bn2_bwd(1)["dRaw2"]
    assert _worst(got, want, bnd) <= 1.0
    got, want, bnd, _, _ = b.bn2_bwd(1, stats=0)["dRaw2"]
    r_bwd = _worst(got, want, bnd)
    got, want, bnd, _, _ = b.bn2_bwd(1, count_mul=3)["dRaw2"]
    r_cnt = _worst(got, want, bnd)
    print(f"[replay-sensitivity] row {step['key']} block {blk} | conv2 forward with pass 0's bn1: {r_fwd:.3g} | bn2 backward with pass 0's "
          f"statistics: {r_bwd:.3g} | bn2 backward with count x 3: {r_cnt:.3g}")
    assert r_fwd > 1.0 and r_bwd > 1.0 and r_cnt > 1.0, (r_fwd, r_bwd, r_cnt)


def test_debug_tap_changes_no_bit():
    """row B from fresh modules, tap off and tap on: the loss and every gradient are the same bits, and so are the forms"""
    out = []
    for tap in (False, True):
        net, model, cls, losses, _ = _run_row("B", tap=tap)
        try:
            out.append((losses, [net.grad(i).cpu() for i in range(len(net.params))], {k: v.detach().cpu() for k, v in model.state_dict().items()},
                        [net.debug_tensor(i, 6)[1] for i in range(8)]))
        finally:
            net.debug_tap(False)
    (l0, g0, s0, f0), (l1, g1, s1, f1) = out
    assert f0 == f1
    assert B.bits_equal(l0, l1)
    assert all(B.bits_equal(a, c) for a, c in zip(g0, g1))
    assert all(torch.equal(s0[k], s1[k]) for k in s0)

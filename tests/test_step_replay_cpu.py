"""CPU-only self-test of the float64 step replay (tests/test_backward_replay_gpu.py): one block of one step is EMULATED here -- every
stage computed in float64 and rounded once to the storage dtype, BatchNorm statistics per pass, running statistics in branch order,
weight and affine gradients summed over the passes -- and handed to the replay in the layout its fixture builds from the debug tap.
The emulation must pass (the chained bounds of the replay hold for a correctly composed step, and its references index the tensors
as the fixture lays them out); the composition faults the replay is there for must fail it."""
import os

import pytest
import torch

import _f64 as B
import step_forms as SF
import test_backward_replay_gpu as T


@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


def st(t, dt):
    return t.float().to(torch.bfloat16) if dt == 1 else t.float()


FAULTS = ("foreign_stats", "count3", "slot", "wgrad_drops_pass", "running_reversed")


def emulate(lib, key, blk, fault=None):
    """-> the dict the replay's `step` fixture builds, holding block `blk` of row `key`.  fault: one composition bug --
    foreign_stats: pass 1's conv2 applies pass 0's bn1;  count3: the BatchNorm backward divides by 3 N oh ow;  slot: the dRaw1 of passes 1
    and 2 land in each other's slot;  wgrad_drops_pass: conv1's weight gradient leaves pass 2 out;  running_reversed: the running
    statistics are updated in reverse branch order"""
    torch.manual_seed(1234)
    dtype, triplet, N, hw = SF.ROWS[key]
    dt = 1 if dtype == "bf16" else 0
    npass = 3 if triplet else 1
    cin, cout, stride = SF.BLOCK_CFG[blk]
    xh, oh = SF.block_dims(hw)[blk]
    word = SF.expected_forms(lib, key)[blk]
    has_ds = stride == 2
    pre = "model.layer%d.%d." % (blk // 2 + 1, blk % 2)
    w1 = st(torch.randn(cout, 3, 3, cin) * 0.05, dt)
    w2 = st(torch.randn(cout, 3, 3, cout) * 0.05, dt)
    wd = st(torch.randn(cout, 1, 1, cin) * 0.1, dt)
    params, before, after, grads = {}, {}, {}, {}
    mods = ["bn1", "bn2"] + (["downsample.1"] if has_ds else [])
    for m in mods:
        params[pre + m + ".weight"] = torch.rand(cout) + 0.5
        params[pre + m + ".bias"] = torch.randn(cout) * 0.1
        before[pre + m + ".running_mean"] = torch.randn(cout) * 0.1
        before[pre + m + ".running_var"] = torch.rand(cout) + 0.5
        after[pre + m + ".running_mean"] = before[pre + m + ".running_mean"].double().clone()
        after[pre + m + ".running_var"] = before[pre + m + ".running_var"].double().clone()
        grads[pre + m + ".weight"] = torch.zeros(cout, dtype=torch.float64)
        grads[pre + m + ".bias"] = torch.zeros(cout, dtype=torch.float64)
    count = N * oh * oh
    bwd_count = count * (3 if fault == "count3" else 1)
    replay = 1 if npass > 1 else 3
    batch = {m: [] for m in mods}          # per pass (mean, unbiased variance): the running statistics follow in branch order

    def finalize(acc, m):
        a = acc.reshape(-1, cout)
        mean, var = a.mean(0), a.var(0, unbiased=False)
        eps = float(torch.tensor(1e-5, dtype=torch.float32))
        invstd = 1 / torch.sqrt(var + eps)
        g, b_ = params[pre + m + ".weight"].double(), params[pre + m + ".bias"].double()
        sc = g * invstd
        sh = b_ - mean * sc
        batch[m].append((mean, var * count / (count - 1)))
        return sc.float(), sh.float(), mean.float(), invstd.float()

    def bnbwd(g, x, bn, m):
        sc, sh, mean, invstd = bn
        gd, xd = g.double(), x.double()
        xm = xd - mean.double()
        s0, s1 = gd.reshape(-1, cout).sum(0), (gd * xm).reshape(-1, cout).sum(0)
        grads[pre + m + ".weight"] += s1 * invstd.double()
        grads[pre + m + ".bias"] += s0
        cB = -sc.double() * invstd.double() ** 2 * s1 / bwd_count
        dx = sc.double() * gd + cB * xd - sc.double() * s0 / bwd_count - cB * mean.double()
        return st(dx, dt)

    P = []
    gw1 = torch.zeros(cout, 3, 3, cin, dtype=torch.float64)
    gw2 = torch.zeros(cout, 3, 3, cout, dtype=torch.float64)
    gwd = torch.zeros(cout, 1, 1, cin, dtype=torch.float64)
    for p in range(npass):
        d = {}
        d["x"] = st(torch.randn(N, xh, xh, cin).clamp_min(0), dt)
        acc1 = B.conv_fwd(d["x"], w1, stride, 1)[2]
        d["raw1"] = st(acc1, dt)
        d["bn1"] = finalize(acc1, "bn1")
        pro = P[0]["bn1"] if fault == "foreign_stats" and p == 1 else d["bn1"]
        a1 = B.xform(d["raw1"], pro[0], pro[1], True, dt)
        acc2 = B.conv_fwd(a1, w2, 1, 1)[2]
        d["raw2"] = st(acc2, dt)
        d["bn2"] = finalize(acc2, "bn2")
        if has_ds:
            accd = B.conv_fwd(d["x"], wd, 2, 0)[2]
            d["rawd"] = st(accd, dt)
            d["bnd"] = finalize(accd, "downsample.1")
            yy = B.bn_act_ref(d["raw2"], d["bn2"][0], d["bn2"][1], res=d["rawd"], rsc=d["bnd"][0], rsh=d["bnd"][1])[0]
        else:
            yy = B.bn_act_ref(d["raw2"], d["bn2"][0], d["bn2"][1], res=d["x"])[0]
        d["y"] = st(yy, dt)
        d["dOut"] = st(torch.randn(N, oh, oh, cout) * 0.01, dt)
        d["G"] = torch.where(d["y"].float() > 0, d["dOut"], torch.zeros((), dtype=d["dOut"].dtype))
        d["dRaw2"] = bnbwd(d["G"], d["raw2"], d["bn2"], "bn2")
        if has_ds:
            d["dRawD"] = bnbwd(d["G"], d["rawd"], d["bnd"], "downsample.1")
        da = B.conv_dgrad(d["dRaw2"], w2, 1, 1, (oh, oh))[0]
        pre1 = d["raw1"].double() * d["bn1"][0].double() + d["bn1"][1].double()
        if word & SF.MASK:
            da = torch.where(pre1 > 0, da, torch.zeros_like(da))
            d["dAct1"] = st(da, dt)
            # the fused mask: bn1's sums come from the dgrad's accumulator, its apply pass reads the stored tensor
            sc, sh, mean, invstd = d["bn1"]
            xm = d["raw1"].double() - mean.double()
            s0, s1 = da.reshape(-1, cout).sum(0), (da * xm).reshape(-1, cout).sum(0)
            grads[pre + "bn1.weight"] += s1 * invstd.double()
            grads[pre + "bn1.bias"] += s0
            cB = -sc.double() * invstd.double() ** 2 * s1 / bwd_count
            d["dRaw1"] = st(sc.double() * d["dAct1"].double() + cB * d["raw1"].double() - sc.double() * s0 / bwd_count - cB * mean.double(), dt)
        else:
            d["dAct1"] = st(da, dt)
            g = torch.where(pre1 > 0, d["dAct1"].double(), torch.zeros_like(da))
            d["dRaw1"] = bnbwd(g, d["raw1"], d["bn1"], "bn1")
        if has_ds:
            d3 = st(B.conv_dgrad(d["dRaw1"], w1, 2, 1, (xh, xh))[0], dt)
            d1 = B.conv_dgrad(d["dRawD"], wd, 2, 0, (xh, xh))[0]
            d["dXin"] = st(d3.double() + d1, dt)
        else:
            d["dXin"] = st(B.conv_dgrad(d["dRaw1"], w1, 1, 1, (xh, xh), residual=d["G"])[0], dt)
        if not (fault == "wgrad_drops_pass" and p == 2):
            gw1 += B.conv_wgrad(d["x"], d["dRaw1"], (cout, 3, 3, cin), stride, 1)[0]
        gw2 += B.conv_wgrad(a1, d["dRaw2"], (cout, 3, 3, cout), 1, 1)[0]
        if has_ds:
            gwd += B.conv_wgrad(d["x"], d["dRawD"], (cout, 1, 1, cin), 2, 0)[0]
        P.append(d)
    grads[pre + "conv1.weight"] = gw1.permute(0, 3, 1, 2).float()
    grads[pre + "conv2.weight"] = gw2.permute(0, 3, 1, 2).float()
    if has_ds:
        grads[pre + "downsample.0.weight"] = gwd.permute(0, 3, 1, 2).float()
    if fault == "slot":
        P[1]["dRaw1"], P[2]["dRaw1"] = P[2]["dRaw1"], P[1]["dRaw1"]
    mom = float(torch.tensor(0.1, dtype=torch.float32))
    for m in mods:
        for mean, unb in (reversed(batch[m]) if fault == "running_reversed" else batch[m]):
            for _ in range(replay):
                after[pre + m + ".running_mean"] = (1 - mom) * after[pre + m + ".running_mean"] + mom * mean
                after[pre + m + ".running_var"] = (1 - mom) * after[pre + m + ".running_var"] + mom * unb
    grads = {k: v.float() for k, v in grads.items()}
    after = {k: v.float() for k, v in after.items()}
    blocks, forms, packs = [None] * 8, [0] * 8, [None] * 8
    blocks[blk], forms[blk] = P, word
    packs[blk] = {"conv1": w1.float(), "conv2": w2.float(), "ds": wd.float()}
    return dict(key=key, dt=dt, npass=npass, N=N, blocks=blocks, forms=forms, packs=packs, params=params, grads=grads, before=before,
                after=after, segs=bool(word & SF.FWD_SEG), losses=None, ratios={})


@pytest.mark.parametrize("key, blk", [("C", 0), ("C", 4), ("E-bf16", 2)], ids=["fp32-triplet-fused-mask", "fp32-triplet-projection", "bf16-projection"])
def test_emulated_step_holds_every_bound(lib, key, blk):
    T.test_step_replay_f64(emulate(lib, key, blk), blk)


def test_emulated_step_is_told_from_foreign_statistics_and_counts(lib):
    T.test_step_replay_sees_foreign_statistics_and_counts(emulate(lib, "C", 0), 0)


@pytest.mark.parametrize("fault", FAULTS)
def test_composition_fault_fails_the_replay(lib, fault):
    stage = dict(foreign_stats="raw2", count3="dRaw2", slot="dRaw1", wgrad_drops_pass="conv1 wgrad", running_reversed="running_mean")[fault]
    with pytest.raises(AssertionError, match=f"row C block 0 .*{stage}"):
        T.test_step_replay_f64(emulate(lib, "C", 0, fault), 0)

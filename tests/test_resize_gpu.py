"""GPU: the resize kernels (csrc/resample.hip through kernels.pil_resize) EQUAL Pillow, byte for byte -- the live Pillow where it imports,
the recorded one (tests/golden/resize_pil.npz) otherwise -- in every form, layout and channel count, with guard bands around every
buffer; PatchDeviceLoader's batches; and the test() drop-ins fed by the loader against the same calls fed with host-built batches."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cases as C  # noqa: E402
from oracle import model as OM  # noqa: E402

import _resize_cases as RC  # noqa: E402
from _inference_util import scale_head  # noqa: E402

DEV = "cuda:0"
SENTINEL = 0xA5


def guarded(shape, pad):
    """a contiguous uint8 device tensor of `shape` inside a buffer filled with SENTINEL, `pad` bytes in front (the tensor's
    alignment) and at least 64 behind; -> (tensor, check) with check() asserting that both bands still hold the sentinel"""
    n = int(np.prod(shape))
    buf = torch.full((pad + n + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    t = buf[pad:pad + n].view(shape)

    def check():
        assert bool((buf[:pad] == SENTINEL).all()) and bool((buf[pad + n:] == SENTINEL).all()), "a guard band was written"
    return t, check


def to_layout(img_hwc, layout):
    """numpy [N, H, W, C] -> the layout's array"""
    return np.ascontiguousarray(img_hwc.transpose(0, 3, 1, 2)) if layout == "chw" else img_hwc


def run(imgs, out_hw, name, box=None, *, layout="hwc", out_layout="hwc", form=None, pads=(64, 64)):
    """imgs: numpy uint8 [N, H, W, C] -> numpy [N, oh, ow, C] through the device, guard bands checked"""
    from ssl_cr_histo_amd import kernels as K
    n, _, _, c = imgs.shape
    src_np = to_layout(imgs, layout)
    x, check_x = guarded(src_np.shape, pads[0])
    x.copy_(torch.from_numpy(src_np))
    oshape = (n, out_hw[0], out_hw[1], c) if out_layout == "hwc" else (n, c, out_hw[0], out_hw[1])
    out, check_out = guarded(oshape, pads[1])
    r = K.pil_resize(x, (out_hw[1], out_hw[0]), name, box=box, out=out, layout=layout, out_layout=out_layout, form=form)
    assert r is out
    torch.cuda.synchronize()
    check_x()
    check_out()
    assert torch.equal(x.cpu(), torch.from_numpy(src_np))                  # the source is only read
    got = out.cpu().numpy()
    return got.transpose(0, 2, 3, 1) if out_layout == "chw" else got


def plan_of(imgs, out_hw, name, box, layout, out_layout):
    from ssl_cr_histo_amd import kernels as K
    n, h, w, c = imgs.shape
    return K.resample_plan((h, w), (out_hw[1], out_hw[0]), name, box=box, n=n, channels=c, layout=layout, out_layout=out_layout)


def forms_of(plan):
    return (None, "fused", "two_pass") if plan["fused_ok"] else (None,)


LAYOUTS = [(a, b) for a in ("hwc", "chw") for b in ("hwc", "chw")]


@pytest.mark.parametrize("name", RC.FILTERS)
@pytest.mark.parametrize("case", RC.CASES, ids=[c[0] for c in RC.CASES])
def test_every_filter_form_layout_and_channel_count_equals_pillow(case, name):
    _, src, out_hw, box = case
    rgb = RC.source(src)
    forms_seen = set()
    for c in (3, 1):
        img = rgb if c == 3 else np.ascontiguousarray(rgb[..., 0])
        want = RC.expected(img, out_hw, name, box, RC.key(src, out_hw, name, box)).reshape(out_hw + (c,))
        for layout, out_layout in LAYOUTS:
            p = plan_of(img.reshape(1, *rgb.shape[:2], c), out_hw, name, box, layout, out_layout)
            forms_seen.add(p["form"])
            for form in forms_of(p):
                got = run(img.reshape(1, *rgb.shape[:2], c), out_hw, name, box, layout=layout, out_layout=out_layout, form=form)
                assert np.array_equal(got[0], want), (case[0], name, c, layout, out_layout, form, p["form"])
    both = box is not None or (out_hw[0] != rgb.shape[0] and out_hw[1] != rgb.shape[1])
    if case[0] == "one":          # -> 1 x 1: ksize = the whole axis, so the wider filters' table slices alone pass the fused LDS budget
        assert forms_seen <= {"fused", "two_pass"} and (name in ("bicubic", "lanczos") or forms_seen == {"fused"})
    else:
        assert forms_seen == ({"fused"} if both else {"horizontal"} if out_hw[0] == rgb.shape[0] else {"vertical"})
    if name in ("bicubic", "lanczos") and src == "bw64":                   # the 0 / 255 image: the overshoot is clipped at both ends
        assert want.min() == 0 and want.max() == 255


@pytest.mark.parametrize("src,out_hw", RC.NEAREST_CASES)
def test_nearest_equals_pillow(src, out_hw):
    rgb = RC.source(src)
    want = RC.expected(rgb, out_hw, "nearest", None, RC.key(src, out_hw, "nearest", None))
    for layout, out_layout in LAYOUTS:
        assert plan_of(rgb[None], out_hw, "nearest", None, layout, out_layout)["form"] == "gather"
        assert np.array_equal(run(rgb[None], out_hw, "nearest", layout=layout, out_layout=out_layout)[0], want)
    l = np.ascontiguousarray(rgb[..., 0])
    assert np.array_equal(run(l[None, ..., None], out_hw, "nearest")[0, ..., 0], want[..., 0])


def test_same_size_without_a_box_is_the_copy_between_layouts():
    rgb = RC.source("r37")
    for layout, out_layout in LAYOUTS:
        assert np.array_equal(run(rgb[None], (37, 53), "bicubic", layout=layout, out_layout=out_layout)[0], rgb)


@pytest.mark.parametrize("n", [0, 1, 5])
def test_batch_sizes_and_repeatability(n):
    from ssl_cr_histo_amd import kernels as K
    rs = np.random.RandomState(300 + n)
    imgs = rs.randint(0, 256, size=(n, 37, 53, 3), dtype=np.uint8)
    for name, out_hw in (("bilinear", (19, 27)), ("lanczos", (37, 27)), ("nearest", (19, 27))):
        for form in ((None, "two_pass") if name == "bilinear" else (None,)):
            got = run(imgs, out_hw, name, layout="hwc", out_layout="chw", form=form)
            assert got.shape == (n,) + out_hw + (3,)
            for i in range(n):
                assert np.array_equal(got[i], RC.expected(imgs[i], out_hw, name)), (n, i, name, form)
            assert np.array_equal(got, run(imgs, out_hw, name, layout="hwc", out_layout="chw", form=form))       # two calls, equal bits
    if n == 0:                                                                 # and without an `out`
        assert K.pil_resize(torch.empty((0, 37, 53, 3), dtype=torch.uint8, device=DEV), (27, 19)).shape == (0, 19, 27, 3)


@pytest.mark.parametrize("name", RC.BOX_FILTERS)
def test_five_boxes_in_one_launch(name):
    """N = 5, every image its own box through table_index: equal to five single calls and to Pillow's resize(box=...)"""
    rs = np.random.RandomState(310)
    imgs = rs.randint(0, 256, size=(5, 37, 53, 3), dtype=np.uint8)
    imgs[0] = RC.source("r37")                                                # the recorded case, for the golden
    boxes = np.array(RC.BOXES5)
    out_hw = (19, 27)
    for layout, out_layout in (("hwc", "chw"), ("chw", "hwc")):
        p = plan_of(imgs, out_hw, name, boxes, layout, out_layout)
        for form in forms_of(p):
            got = run(imgs, out_hw, name, boxes, layout=layout, out_layout=out_layout, form=form)
            for i in range(5):
                single = run(imgs[i:i + 1], out_hw, name, RC.BOXES5[i], layout=layout, out_layout=out_layout, form=form)
                assert np.array_equal(got[i], single[0]), (i, form)
                k = RC.key("r37", out_hw, name, RC.BOXES5[i]) if i == 0 else None
                assert np.array_equal(got[i], RC.expected(imgs[i], out_hw, name, RC.BOXES5[i], k)), (i, form)
    # a box repeated: two images share a table set
    rep = boxes[[1, 3, 1, 1, 3]]
    got = run(imgs, out_hw, name, rep)
    for i in range(5):
        assert np.array_equal(got[i], RC.expected(imgs[i], out_hw, name, tuple(rep[i])))


@pytest.mark.parametrize("hw,out_hw", RC.BIG_CASES)
def test_large_down_scale_takes_the_plans_own_choice(hw, out_hw):
    """8192 x 8 -> 8 x 8 LANCZOS (ksize 6145) through the plan's choice: the single horizontal launch, since the 8 -> 8 axis is
    skipped; with 9 rows both passes are needed and the plan picks the two-launch form -- the fused tile cannot hold 8192 columns"""
    img = RC.big_source(*hw)
    p = plan_of(img[None], out_hw, "lanczos", None, "hwc", "chw")
    assert p["form"] == ("horizontal" if hw[0] == out_hw[0] else "two_pass") and not p["fused_ok"]
    want = RC.expected(img, out_hw, "lanczos", None, RC.key(f"big{hw[0]}x{hw[1]}", out_hw, "lanczos", None))
    for layout, out_layout in (("hwc", "chw"), ("chw", "hwc")):
        assert np.array_equal(run(img[None], out_hw, "lanczos", layout=layout, out_layout=out_layout)[0], want)


@pytest.mark.parametrize("pads", [(65, 67), (66, 65), (67, 66)])
def test_buffers_at_every_alignment(pads):
    """source and destination bases that are no multiple of 4: whole-dword loads and stores at the row ends must stay inside"""
    rgb = RC.source("r37")
    for name, out_hw in (("bilinear", (19, 27)), ("bicubic", (19, 28)), ("hamming", (37, 27)), ("box", (19, 53))):
        want = RC.expected(rgb, out_hw, name)
        for layout, out_layout in LAYOUTS:
            for form in forms_of(plan_of(rgb[None], out_hw, name, None, layout, out_layout)):
                got = run(rgb[None], out_hw, name, layout=layout, out_layout=out_layout, form=form, pads=pads)
                assert np.array_equal(got[0], want), (name, out_hw, layout, out_layout, form)


def test_more_than_one_tile_and_a_ragged_edge():
    """150 x 200 -> 70 x 130: three tiles across, five down, both edges ragged; and 256 x 256 -> 128 x 128, the eval shape's ratio"""
    rs = np.random.RandomState(320)
    for (h, w), out_hw in (((150, 200), (70, 130)), ((256, 256), (128, 128)), ((40, 50), (100, 139))):
        imgs = rs.randint(0, 256, size=(2, h, w, 3), dtype=np.uint8)
        for name in ("bilinear", "lanczos"):
            want = np.stack([RC.expected(im, out_hw, name) for im in imgs])
            p = plan_of(imgs, out_hw, name, None, "hwc", "chw")
            assert p["form"] == "fused" and p["grid"][0] > 2
            for form in (None, "two_pass"):
                for layout, out_layout in (("hwc", "chw"), ("chw", "hwc")):
                    assert np.array_equal(run(imgs, out_hw, name, layout=layout, out_layout=out_layout, form=form), want), (h, w, name, form)


def test_argument_errors():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    x = torch.zeros((1, 9, 7, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.SslcrError):
        K.pil_resize(x.float(), (4, 4))
    with pytest.raises(L.SslcrError):
        K.pil_resize(x, (4, 4), layout="chw")                       # 9 channels
    with pytest.raises(L.SslcrError):
        K.pil_resize(x, (4, 4), out=torch.zeros((1, 4, 4, 1), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        K.pil_resize(x, (4, 4), "nearest", box=(0, 0, 3, 3))
    with pytest.raises(ValueError):
        K.pil_resize(x, (4, 0))
    with pytest.raises(L.SslcrError, match="fused"):
        K.pil_resize(torch.zeros((1, 9, 8192, 3), dtype=torch.uint8, device=DEV), (8, 8), "lanczos", form="fused")


# ---------------------------------------------------------------------------------------------------------------- the loader
def host_batches(patches, image_size, batch_size, targets, name="bilinear"):
    """the host loader's batches: transforms.Resize(image_size) on a PIL image (Pillow bilinear), then permute(2, 0, 1)"""
    from ssl_cr_histo_amd import kernels as K
    oh, ow = K.resize_output_size(patches.shape[1], patches.shape[2], image_size)
    tiles = np.stack([RC.expected(p, (oh, ow), name) for p in patches]).transpose(0, 3, 1, 2)
    tiles = torch.from_numpy(np.ascontiguousarray(tiles))
    return [(tiles[i:i + batch_size],) + tuple(torch.as_tensor(t)[i:i + batch_size] for t in targets) for i in range(0, len(patches), batch_size)]


def test_patch_loader_yields_the_host_loaders_batches():
    from ssl_cr_histo_amd.inference import PatchDeviceLoader
    c = RC.LOADER
    patches = RC.loader_patches()
    ta, tb = np.arange(10, dtype=np.float32), -np.arange(10, dtype=np.float32)
    want = host_batches(patches, c["image_size"], c["batch_size"], (ta, tb))
    for layout, arr in (("hwc", patches), ("chw", np.ascontiguousarray(patches.transpose(0, 3, 1, 2)))):
        loader = PatchDeviceLoader(arr, ta, tb, image_size=c["image_size"], batch_size=c["batch_size"], layout=layout, device=DEV)
        for _ in range(2):                                         # iterable more than once; the upload happens once
            got = list(loader)
            assert len(got) == len(loader) == len(want) == 3
            for g, w in zip(got, want):
                assert g[0].is_cuda and g[0].dtype == torch.uint8 and tuple(g[0].shape[1:]) == (3, 32, 32)
                assert torch.equal(g[0].cpu(), w[0]) and torch.equal(g[1], w[1]) and torch.equal(g[2], w[2])
        assert loader.patches.is_cuda


def _engine(dtype):
    from ssl_cr_histo_amd import engine as E
    idx = torch.device(DEV).index
    cur = E._engines.get(idx)
    if cur is None or cur.dtype != E._DTYPES[dtype]:
        E._engines.pop(idx, None)
        E.set_engine(E.Engine(DEV, dtype))
    return E.get_engine(DEV)


def _build(classes, head_scale=1.0):
    from ssl_cr_histo_amd import net
    model, cls = net.TripletNet_Finetune("resnet18"), net.FinetuneResNet(classes)
    model.load_state_dict(OM.init_state(C.PARAM_SEED, OM.net_param_specs(), random_running_stats=True))
    cls.load_state_dict(OM.init_state(C.PARAM_SEED + 1, OM.classifier_param_specs("finetune", classes)))
    scale_head(cls, head_scale)
    return model.to(DEV), cls.to(DEV)


def _ns(**kw):
    return types.SimpleNamespace(print_freq=0, **kw)


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bpq_test_fed_by_the_loader_returns_the_bits_of_the_host_fed_call(dtype):
    """11 patches of 128 x 128, Resize(64), batches of 4: bpq_test fed by PatchDeviceLoader against the same call fed with the
    host-built batches (Pillow bilinear, permute(2, 0, 1)) -- outputs and features bit for bit"""
    from ssl_cr_histo_amd import steps
    from ssl_cr_histo_amd.inference import PatchDeviceLoader
    _engine(dtype)
    model, cls = _build(1)
    patches = np.random.RandomState(330).randint(0, 256, size=(11, 128, 128, 3), dtype=np.uint8)
    ta, tb = C.f32(331, (11,)), C.f32(332, (11,))
    host = host_batches(patches, 64, 4, (ta, tb))
    a = steps.bpq_test(_ns(), model, cls, host)
    b = steps.bpq_test(_ns(), model, cls, PatchDeviceLoader(patches, ta, tb, image_size=64, batch_size=4, device=DEV))
    assert a[0].shape == (11,) and a[1].shape == (11, 768) and a[1].std() > 0
    for u, v in zip(a, b):
        assert not v.is_cuda and _bits(u, v)
    b2 = steps.bpq_sup_test(_ns(), model, cls, torch.nn.MSELoss(), PatchDeviceLoader(patches, ta, tb, image_size=64, batch_size=4, device=DEV))
    assert all(_bits(u, v) for u, v in zip(a, b2))


def test_kather_cr_test_fed_by_the_loader_returns_the_bits_of_the_host_fed_call():
    """11 patches of 128 x 128 to 96 x 96 (a non-integer scale), bf16 mode: predictions, targets and scores"""
    from ssl_cr_histo_amd import steps
    from ssl_cr_histo_amd.inference import PatchDeviceLoader
    _engine("bf16")
    model, cls = _build(9, 0.05)
    patches = np.random.RandomState(340).randint(0, 256, size=(11, 128, 128, 3), dtype=np.uint8)
    y = C.ints(341, (11,), 9)
    a = steps.kather_cr_test(_ns(), model, cls, host_batches(patches, 96, 4, (y,)))
    b = steps.kather_cr_test(_ns(), model, cls, PatchDeviceLoader(patches, y, image_size=96, batch_size=4, device=DEV))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[1], y) and _bits(a[2], b[2])
    assert a[2].shape == (11, 9) and a[2].std() > 0

"""Drop-in ``train()`` / ``validate()`` for the reference scripts, same signatures and return tuples, running every
iteration as ONE native engine step (teacher fwd + student fwd + losses + backward + all-reduce) plus one fused
optimizer launch.  Loaders are any iterables yielding the reference's batch tuples, uint8 or float,
CPU or GPU.  Differences from the reference loops that do not change results: no per-iteration ``.item()`` host syncs
(meters are filled from device scalars at print/epoch boundaries) and features are concatenated once, not per step.

Gradient accumulation: every ``*_train`` reads ``k = getattr(args, "micro_batches", 1)`` (``validate()`` functions ignore it).  With
k > 1 each loader batch is cut into k contiguous micro-batches (``micro_ranges``; labeled and unlabeled rows separately), micro-step j
runs with the FULL batch's counts as its global counts and adds its gradients to those of the steps before it (j > 0), and ONE
optimizer step (with ``args.clip_grad_norm`` on the accumulated gradient) follows: the reference's global batch on a card that cannot
hold it.  The return tuples keep their shapes.  What this is, exactly:
  * train-mode BatchNorm uses each micro-batch's own statistics -- the reference's per-replica statistics under ``nn.DataParallel``;
  * running statistics and ``num_batches_tracked`` are updated by every micro-step in turn, as k successive torch forwards would
    (``DataParallel`` keeps replica 0's only);
  * the first micro-step of a batch clears the buffer; anybody who calls the engine with ``accumulate=True`` on a buffer left from
    before an optimizer step adds to that stale gradient, as torch does without ``zero_grad``.

Loss options: every ``*_train`` and ``*_validate`` with a cross-entropy loss reads ``getattr(args, "loss_options", None)``, a
``LossOptions`` (class weights, label smoothing, ignore_index; FixMatch threshold and UDA temperature of the consistency term); absent,
None or all-default: the code path of every earlier version.  The MSE loops (``bpq_*``) raise ValueError for anything else.  A
weighted or ignore-index mean divides by the sum of w[y] over the kept rows of the WHOLE global batch: ``denominator_plan`` says when
that sum needs a launch of its own (any option set, and micro-batches or ranks: once per loader batch, from the full batch's
targets) and a 2-float all-reduce (ranks); one rank with k = 1 needs neither, the loss kernel sums its own rows.  The CR training loops leave
``args.loss_stats`` = dict(rows, confident, mask_rate, mean_max_prob) of the epoch's unlabeled rows (one read at the epoch's end).

reference                                   here
eval_BreastPathQ_SSL_CR.train/validate      bpq_cr_train / bpq_cr_validate      (:37-128 / :131-175)
eval_Camelyon_SSL_CR.train/validate         cam_cr_train / cam_cr_validate      (:33-157 / :160-225)
eval_Kather_SSL_CR.train/validate           kather_cr_train / kather_cr_validate(:37-127 / :130-179)
pretrain_BreastPathQ|Camelyon16|RSP.train   rsp_train / rsp_validate            (:27-92 / :95-148)
eval_Camelyon_SSL.train                     cam_sup_train                       (:31-119)
eval_BreastPathQ_SSL.train                  bpq_sup_train                       (:35-103)
eval_Kather_SSL.train/validate              kather_sup_train / kather_sup_validate (:32-99 / :102-151)
eval_BreastPathQ_SSL_CR.test                bpq_test                            (:178-242)
eval_BreastPathQ_SSL.test                   bpq_sup_test                        (:152-216)
eval_Kather_SSL_CR.test                     kather_cr_test                      (:182-245)
eval_Kather_SSL.test                        kather_sup_test                     (:154-213)
test_Camelyon16.test                        camelyon16_test                     (:30-70)

The ``*_test`` functions keep everything on the device until ONE copy at the end: predictions and softmax scores come from
sslcr_predict, which also counts the confusion matrix of the classification variants (``last_test_confusion()``, the input of
``inference.metrics_from_confusion``); loss and accuracy go through the validate() step and the meters, read at print boundaries only.
"""
import time

import torch

from .dist import shard_range
from .engine import get_engine
from .kernels import LossOptions, ce_denominator
from .util import AverageMeter


class _Meters:
    """AverageMeter semantics (util.py:26-46) fed from device scalars without a sync per step.

    Sharded runs (one process per GPU): a step's losses are THIS rank's share -- already scaled by 1/global-count, so the SUM
    over ranks is the global value -- and stay local until somebody looks: meters() issues ONE all-reduce of all rows gathered so
    far ("one small all-reduce per print_freq"), on the engine's own communicator, and only then syncs to the
    host.  `reduce` is that in-place SUM over ranks (None on one rank), `world` scales the meter weights to global counts."""

    def __init__(self, names, reduce=None, world=1, device=None):
        self.names = names
        self.device = device                # where the row-count header lives when no row has been added yet
        self.rows, self.weights = [], []
        self.reduce, self.world = reduce, world
        self.done = []                      # rows already reduced and fetched: python lists

    def add(self, losses, n):
        self.rows.append(losses)
        self.weights.append(n * self.world)

    def meters(self, acc_denoms=None):
        """COLLECTIVE on sharded runs: every rank must call it at the same points with the same number of rows gathered since
        its last call (the step functions do: print_freq boundaries and epoch end of equally long loaders).  A rank whose loader
        is shorter would otherwise reduce a buffer of another length -- a hang or mismatched sums -- so a fixed-size header with
        the row count is reduced first and a disagreement raises on every rank."""
        out = {k: AverageMeter() for k in self.names}
        if self.reduce is not None:
            # the count's three base-256 DIGITS and their squares: all ranks hold the same n  <=>  W * sum(d^2) == (sum d)^2 for every
            # digit (Cauchy-Schwarz with equality).  A square is at most 255^2 and a sum over ranks at most W * 255^2 < 2^24 for
            # W <= 256, so every partial sum of any reduction order is an exact fp32 integer (with base-4096 digits the cross-rank
            # sums of squares passed 2^24 and could round: a false mismatch at world >= 3)
            n = len(self.rows)
            if self.world > 256:
                raise RuntimeError("_Meters.meters(): the row-count header is exact in fp32 for world <= 256 only")
            if n >= 1 << 24:
                raise RuntimeError("_Meters.meters(): more than 2^24 rows gathered between two reads")
            d = [float((n >> (8 * i)) & 255) for i in range(3)]
            dev = self.rows[0].device if self.rows else self.device
            hdr = torch.tensor(d + [x * x for x in d], dtype=torch.float32, device=dev)
            self.reduce(hdr)
            h = hdr.cpu().tolist()
            if any(h[3 + i] * self.world != h[i] * h[i] for i in range(3)):
                mean = sum(h[i] * 256 ** i for i in range(3)) / self.world
                raise RuntimeError(f"_Meters.meters(): the ranks gathered different numbers of steps since the last read (this rank "
                                   f"{n}, mean over ranks {mean:g}): the loaders' lengths differ, or "
                                   f"meters() was not called on every rank")
        if self.rows:
            vals = torch.stack(self.rows)
            if self.reduce is not None:
                self.reduce(vals)                                  # the one data collective per print / epoch boundary
            self.done += vals.cpu().tolist()                       # the device->host sync
            self.rows = []
        for r, n in zip(self.done, self.weights):
            for k in self.names:
                if k == "acc":
                    out[k].update(r[3] / n, n)
                else:
                    out[k].update(r[{"loss": 0, "loss_x": 1, "loss_u": 2}[k]], n)
        return out


def _meters(eng, names):
    return _Meters(names, eng.all_reduce_sum if eng.world > 1 else None, eng.world, eng.device)


def _prefetch_on(args):
    import os
    return bool(getattr(args, "device_prefetch", False)) or os.environ.get("SSLCR_PREFETCH", "0") not in ("", "0")


def _ahead(batches, eng, enabled):
    """Host-fed loaders: move batch k+1's image tensors (dim >= 4, still in host memory) to the device on a copy stream while
    step k runs, so the PCIe copy (214 MB per benchmark step = 4.3 ms at 50 GB/s, tools/pcie_inclusive.py) hides under compute.
    Everything else in a batch (targets, WSI tile coordinates) is left where it is.  OFF unless ``args.device_prefetch`` or
    SSLCR_PREFETCH=1: it calls ``next(loader)`` one step early, which reorders the loader's random draws against the step's own
    (``torch.randperm`` in the Camelyon loop) when both use the main process's generators -- harmless with DataLoader workers
    (they draw from their own), a different random stream than the reference's with ``num_workers=0``."""
    if not enabled:
        yield from batches
        return
    dev = eng.device
    copy = eng.copy_stream()

    def move(obj, moved):
        if torch.is_tensor(obj):
            if obj.dim() >= 4 and not obj.is_cuda:
                t = obj.to(dev, non_blocking=True)
                moved.append(t)
                return t
            return obj
        if isinstance(obj, (tuple, list)):
            return type(obj)(move(o, moved) for o in obj)
        return obj

    it = iter(batches)

    def fetch():
        try:
            b = next(it)
        except StopIteration:
            return None
        moved = []
        with torch.cuda.stream(copy):
            mb = move(b, moved)
            ev = torch.cuda.Event()
            ev.record(copy)
        return mb, ev, moved

    nxt = fetch()
    while nxt is not None:
        cur, ev, moved = nxt
        nxt = fetch()                                   # batch k+1's copies are queued before step k is launched
        st = torch.cuda.current_stream(dev)
        st.wait_event(ev)
        for t in moved:
            t.record_stream(st)                         # allocated on the copy stream, consumed on the compute stream
        yield cur


def micro_ranges(n, k):
    """[(lo, hi)] * k: the contiguous micro-batches of a batch of n rows -- ``dist.shard_range(n, j, k)``, remainders to the lowest
    (a micro-batch is a shard in time).  Pure host logic.  k > n (an empty micro-batch) raises ValueError."""
    k = int(k)
    if k < 1 or k > n:
        raise ValueError(f"micro_batches = {k} does not cut a batch of {n} rows into non-empty micro-batches")
    return [shard_range(n, j, k) for j in range(k)]


def _micro_k(args):
    """args.micro_batches; absent (or None) = 1: one engine step per loader batch, the code path of every earlier version."""
    k = getattr(args, "micro_batches", 1)
    return 1 if k is None else int(k)


def _sum_losses(parts):
    # micro-step j's losses are its share of the global-batch values (scaled by 1 / global count), #correct a count: both add.
    # On the device, no host sync
    return torch.stack([p["losses"] for p in parts]).sum(0)


def _loss_options(args, mse=None):
    """args.loss_options; absent, None or all-default = None: the code path of every earlier version.  mse: the name of a loop whose
    loss is F.mse_loss, which has no options."""
    o = getattr(args, "loss_options", None)
    if o is None:
        return None
    if not isinstance(o, LossOptions):
        raise TypeError(f"args.loss_options must be a LossOptions (got {type(o).__name__})")
    if o.is_default():
        return None
    if mse is not None:
        raise ValueError(f"{mse}: args.loss_options = {o!r} -- the loss of this loop is F.mse_loss, which has no such options")
    return o


def denominator_plan(opts, k, world):
    """-> (launch, all_reduce): does a loader batch need a denominator launch of its own (sslcr_ce_denominator over the full batch's
    targets) and an all-reduce of it?  Pure host logic.  Never for absent or all-default options.  With any option set the divisor
    of 'mean' is the kept rows' weight over the WHOLE global batch (class weights, an ignore_index, or just rows labelled -100,
    which are left out once an option is set), and a step that holds only part of it -- a micro-batch (k > 1) or a shard
    (world > 1) -- cannot derive that from its own rows; one rank with k = 1 can, and nothing is added."""
    if opts is None or not opts.needs_denominator() or (k == 1 and world == 1):
        return False, False
    return True, world > 1


def _denominator(eng, opts, y, ncls, k):
    """the supervised term's divisor over the global batch, on the device (None where the loss kernel's own rows are the batch)"""
    launch, reduce = denominator_plan(opts, k, eng.world)
    if not launch:
        return None
    den = ce_denominator(y.to(eng.device).long().reshape(-1).contiguous(), ncls, opts.weight_on(eng.device, ncls), opts.ignore_index)
    return eng.all_reduce_sum(den) if reduce else den


def _loss_kw(eng, opts, y, ncls, k):
    return {} if opts is None else dict(loss_options=opts, denominator=_denominator(eng, opts, y, ncls, k))


class _MaskStats:
    """{#confident unlabeled rows, sum of the teacher's max-probs, #unlabeled rows} of an epoch's steps, kept on the device until
    the epoch's end"""

    def __init__(self, eng, args, opts):
        self.eng, self.args, self.rows, self.n = eng, args, [], 0
        self.on = opts is not None

    def add(self, r, nu):
        if self.on:
            self.rows.append(r["stats"])
            self.n += nu

    def finish(self):
        """COLLECTIVE when sharded, as meters(): every rank of a run with options calls it once per epoch, whatever it gathered; the
        row count travels in the reduced vector, so ranks need not have seen equally many rows"""
        if not self.on:
            return
        tot = torch.zeros(3, dtype=torch.float32, device=self.eng.device)
        if self.rows:
            tot[:2] = torch.stack(self.rows).sum(0)
        tot[2] = float(self.n)
        conf, maxp, n = self.eng.all_reduce_sum(tot).cpu().tolist()
        n = int(n)
        self.args.loss_stats = dict(rows=n, confident=int(conf), mask_rate=conf / n if n else float("nan"),
                                    mean_max_prob=maxp / n if n else float("nan"))


def _ssl_cr_step(eng, te, st, kind, x, y, u_w, u_s, lambda_u, k, opts=None):
    """one loader batch of a consistency-training loop as k accumulated micro-steps (k == 1: the plain engine step).  Rows of the
    returned feats / logits / logits_t are in the order the single step returns them: all labeled rows, then all unlabeled.
    opts: the loop's LossOptions (None: none); the denominator of a weighted / ignore-index mean is taken ONCE, over the full
    batch's targets, and handed to every micro-step."""
    kw = _loss_kw(eng, opts, y, st.ncls, k)
    if k == 1:
        return eng.step_ssl_cr(te, st, kind, x, y, u_w, u_s, lambda_u, **kw)
    nx, nu = x.shape[0], u_w.shape[0]
    if k > nx or k > nu:
        raise ValueError(f"micro_batches = {k} exceeds the batch: nx = {nx} labeled, nu = {nu} unlabeled rows")
    parts = []
    for j, ((a, b), (c, d)) in enumerate(zip(micro_ranges(nx, k), micro_ranges(nu, k))):
        parts.append(eng.step_ssl_cr(te, st, kind, x[a:b], y[a:b], u_w[c:d], u_s[c:d], lambda_u, nx_global=nx * eng.world,
                                     nu_global=nu * eng.world, accumulate=j > 0, **kw))
    nxj = [b - a for a, b in micro_ranges(nx, k)]                    # a part's rows: its nxj labeled ones, then its unlabeled ones
    out = {key: torch.cat([p[key][:n] for p, n in zip(parts, nxj)] + [p[key][n:] for p, n in zip(parts, nxj)]) for key in ("feats", "logits")}
    out["logits_t"] = torch.cat([p["logits_t"] for p in parts])
    out["losses"] = _sum_losses(parts)
    if opts is not None:
        out["stats"] = torch.stack([p["stats"] for p in parts]).sum(0)
    return out


def _sup_step(eng, net, kind, xs, y, k, opts=None):
    """one loader batch of a student-only training loop as k accumulated micro-steps (k == 1: the plain engine step)."""
    kw = _loss_kw(eng, opts, y, net.ncls, k)
    if k == 1:
        return eng.step_supervised(net, kind, xs, y, train=True, **kw)
    n = xs[0].shape[0]
    if k > n:
        raise ValueError(f"micro_batches = {k} exceeds the batch: n = {n} rows")
    parts = [eng.step_supervised(net, kind, [x[a:b] for x in xs], y[a:b], train=True, n_global=n * eng.world, accumulate=j > 0, **kw)
             for j, (a, b) in enumerate(micro_ranges(n, k))]
    return dict(losses=_sum_losses(parts), feats=torch.cat([p["feats"] for p in parts]), logits=torch.cat([p["logits"] for p in parts]))


def _val_step(eng, net, xs, y, opts):
    """one validate() batch with a cross-entropy loss (eval-mode forward + loss, no backward)"""
    return eng.step_supervised(net, "ce", xs, y, train=False, **_loss_kw(eng, opts, y, net.ncls, 1))


def _device_of(model):
    return next(model.parameters()).device


def _maybe_print(args, batch_idx, tag, epoch, total, t0, meters):
    pf = getattr(args, "print_freq", 0)
    if pf and (batch_idx + 1) % pf == 0:
        m = meters.meters()
        body = "\t".join(f"{k} {v.val:.3f} ({v.avg:.3f})" for k, v in m.items())
        print(f"{tag}: [{epoch}][{batch_idx + 1}/{total}]\tBT {(time.time() - t0) / (batch_idx + 1):.3f}\t{body}")


def _len(x):
    try:
        return len(x)
    except TypeError:
        return -1


# ------------------------------------------------------------------------------------------------ BreastPathQ SSL_CR
def bpq_cr_train(args, model_teacher, model_student, classifier_teacher, classifier_student, labeled_train_loader,
                 unlabeled_train_loader, optimizer, epoch):
    """eval_BreastPathQ_SSL_CR.train: returns (loss_avg, loss_x_avg, loss_u_avg, final_feats, final_targets)."""
    _loss_options(args, mse="bpq_cr_train")
    eng = get_engine(_device_of(model_student))
    for m in (model_teacher, classifier_teacher):
        m.eval()
    for m in (model_student, classifier_student):
        m.train()
    te, st = eng.bind(model_teacher, classifier_teacher), eng.bind(model_student, classifier_student)
    meters = _meters(eng, ["loss", "loss_x", "loss_u"])
    feats, targets = [], []
    k = _micro_k(args)
    t0 = time.time()
    for batch_idx, (data_x, data_u) in enumerate(_ahead(zip(labeled_train_loader, unlabeled_train_loader), eng, _prefetch_on(args))):
        inputs_x, targets_x = data_x
        inputs_u_w, inputs_u_s = data_u
        inputs_x = inputs_x.reshape(-1, 3, 256, 256)                         # :74 (hard-coded by the reference)
        targets_x = targets_x.float().to(eng.device)
        r = _ssl_cr_step(eng, te, st, "mse", inputs_x, targets_x.reshape(-1), inputs_u_w, inputs_u_s, args.lambda_u, k)
        st.optimizer_step(optimizer, max_grad_norm=getattr(args, "clip_grad_norm", None))
        meters.add(r["losses"], inputs_x.shape[0])
        feats.append(r["feats"])
        targets.append(targets_x)
        _maybe_print(args, batch_idx, "Train", epoch, _len(labeled_train_loader), t0, meters)
    m = meters.meters()
    return m["loss"].avg, m["loss_x"].avg, m["loss_u"].avg, torch.cat(feats).detach(), torch.cat(targets).detach()


def bpq_cr_validate(args, model_student, classifier_student, val_loader, epoch):
    """eval_BreastPathQ_SSL_CR.validate -> loss_avg."""
    _loss_options(args, mse="bpq_cr_validate")
    eng = get_engine(_device_of(model_student))
    model_student.eval()
    classifier_student.eval()
    st = eng.bind(model_student, classifier_student)
    meters = _meters(eng, ["loss"])
    t0 = time.time()
    for batch_idx, (input, target) in enumerate(_ahead(val_loader, eng, _prefetch_on(args))):
        r = eng.step_supervised(st, "mse", [input], target.float().reshape(-1), train=False)
        meters.add(r["losses"], target.size(0))
        _maybe_print(args, batch_idx, "Val", epoch, _len(val_loader), t0, meters)
    return meters.meters()["loss"].avg


# ------------------------------------------------------------------------------------------------ Camelyon16 SSL_CR
def _cat_shuffle(a, b, perm):
    return torch.cat([a, b])[perm]


def cam_cr_train(args, model_teacher, model_student, classifier_teacher, classifier_student, tumor_labeled_train_loader,
                 normal_labeled_train_loader, tumor_unlabeled_train_loader, normal_unlabeled_train_loader, optimizer, epoch):
    """eval_Camelyon_SSL_CR.train: returns (loss, loss_x, loss_u, acc, final_feats[:labeled], final_targets)."""
    eng = get_engine(_device_of(model_student))
    for m in (model_teacher, classifier_teacher):
        m.eval()
    for m in (model_student, classifier_student):
        m.train()
    te, st = eng.bind(model_teacher, classifier_teacher), eng.bind(model_student, classifier_student)
    meters = _meters(eng, ["loss", "loss_x", "loss_u", "acc"])
    feats, targets = [], []
    k = _micro_k(args)
    opts = _loss_options(args)
    mask = _MaskStats(eng, args, opts)
    t0 = time.time()
    S = args.image_size
    loaders = zip(tumor_labeled_train_loader, normal_labeled_train_loader, tumor_unlabeled_train_loader,
                  normal_unlabeled_train_loader)
    for batch_idx, (tumor_data_x, normal_data_x, tumor_data_u, normal_data_u) in enumerate(_ahead(loaders, eng, _prefetch_on(args))):
        t_x, t_y = tumor_data_x
        n_x, n_y = normal_data_x
        t_x, t_y = t_x.reshape(-1, 3, S, S), t_y.reshape(-1)
        n_x, n_y = n_x.reshape(-1, 3, S, S), n_y.reshape(-1)
        t_uw, t_us = tumor_data_u
        n_uw, n_us = normal_data_u
        p_x = torch.randperm(2 * len(t_x))                       # same three draws, same order as :79-81
        p_uw = torch.randperm(2 * len(t_uw))
        p_us = torch.randperm(2 * len(t_us))
        x, y = _cat_shuffle(t_x, n_x, p_x.to(t_x.device)), _cat_shuffle(t_y, n_y, p_x.to(t_y.device)).long()
        u_w, u_s = _cat_shuffle(t_uw, n_uw, p_uw.to(t_uw.device)), _cat_shuffle(t_us, n_us, p_us.to(t_us.device))
        r = _ssl_cr_step(eng, te, st, "ce", x, y, u_w, u_s, args.lambda_u, k, opts)
        st.optimizer_step(optimizer, max_grad_norm=getattr(args, "clip_grad_norm", None))
        n = x.shape[0]
        meters.add(r["losses"], n)
        mask.add(r, u_w.shape[0])
        feats.append(r["feats"][:n])
        targets.append(y.to(eng.device))
        _maybe_print(args, batch_idx, "Train", epoch, _len(tumor_labeled_train_loader) * 2, t0, meters)
    m = meters.meters()
    mask.finish()
    return m["loss"].avg, m["loss_x"].avg, m["loss_u"].avg, m["acc"].avg, torch.cat(feats).detach(), torch.cat(targets).detach()


def cam_cr_validate(args, model_student, classifier_student, val_tumor_loader, val_normal_loader, epoch):
    """eval_Camelyon_SSL_CR.validate -> (loss_avg, acc_avg)."""
    eng = get_engine(_device_of(model_student))
    model_student.eval()
    classifier_student.eval()
    st = eng.bind(model_student, classifier_student)
    meters = _meters(eng, ["loss", "acc"])
    opts = _loss_options(args)
    t0 = time.time()
    for batch_idx, (data_tumor, data_normal) in enumerate(_ahead(zip(val_tumor_loader, val_normal_loader), eng, _prefetch_on(args))):
        t_x, t_y = data_tumor
        n_x, n_y = data_normal
        perm = torch.randperm(2 * len(t_x))
        x = torch.cat([t_x, n_x])[perm.to(t_x.device)]
        y = torch.cat([t_y, n_y])[perm.to(t_y.device)].long()
        r = _val_step(eng, st, [x], y, opts)
        meters.add(r["losses"], y.size(0))
        _maybe_print(args, batch_idx, "Val", epoch, 2 * _len(val_tumor_loader), t0, meters)
    m = meters.meters()
    return m["loss"].avg, m["acc"].avg


# ------------------------------------------------------------------------------------------------ Kather SSL_CR
def kather_cr_train(args, model_teacher, model_student, classifier_teacher, classifier_student, labeled_train_loader,
                    unlabeled_train_loader, optimizer, epoch):
    """eval_Kather_SSL_CR.train: CE + hard-pseudo-label CE, single labeled/unlabeled loader pair;
    returns (loss, loss_x, loss_u, acc)."""
    eng = get_engine(_device_of(model_student))
    for m in (model_teacher, classifier_teacher):
        m.eval()
    for m in (model_student, classifier_student):
        m.train()
    te, st = eng.bind(model_teacher, classifier_teacher), eng.bind(model_student, classifier_student)
    meters = _meters(eng, ["loss", "loss_x", "loss_u", "acc"])
    k = _micro_k(args)
    opts = _loss_options(args)
    mask = _MaskStats(eng, args, opts)
    t0 = time.time()
    for batch_idx, (data_x, data_u) in enumerate(_ahead(zip(labeled_train_loader, unlabeled_train_loader), eng, _prefetch_on(args))):
        inputs_x, targets_x = data_x
        inputs_u_w, inputs_u_s = data_u
        inputs_x = inputs_x.reshape(-1, 3, 256, 256)                          # :68
        targets_x = targets_x.reshape(-1).long()                              # :69
        r = _ssl_cr_step(eng, te, st, "ce", inputs_x, targets_x, inputs_u_w, inputs_u_s, args.lambda_u, k, opts)
        st.optimizer_step(optimizer, max_grad_norm=getattr(args, "clip_grad_norm", None))
        meters.add(r["losses"], inputs_x.shape[0])
        mask.add(r, inputs_u_w.shape[0])
        _maybe_print(args, batch_idx, "Train", epoch, _len(labeled_train_loader), t0, meters)
    m = meters.meters()
    mask.finish()
    return m["loss"].avg, m["loss_x"].avg, m["loss_u"].avg, m["acc"].avg


def kather_cr_validate(args, model_student, classifier_student, val_loader, epoch):
    """eval_Kather_SSL_CR.validate -> (loss_avg, acc_avg)."""
    eng = get_engine(_device_of(model_student))
    model_student.eval()
    classifier_student.eval()
    st = eng.bind(model_student, classifier_student)
    meters = _meters(eng, ["loss", "acc"])
    opts = _loss_options(args)
    for batch_idx, (input, target) in enumerate(_ahead(val_loader, eng, _prefetch_on(args))):
        r = _val_step(eng, st, [input], target.reshape(-1).long(), opts)
        meters.add(r["losses"], target.size(0))
    m = meters.meters()
    return m["loss"].avg, m["acc"].avg


# ------------------------------------------------------------------------------------------------ RSP pretraining
def _plain_ce(criterion, where):
    """the engine computes plain mean cross-entropy (what the reference's nn.CrossEntropyLoss() is): anything else -- class
    weights, label smoothing, a non-default ignore_index or reduction -- must not be silently dropped."""
    if criterion is None:
        return
    if not isinstance(criterion, torch.nn.CrossEntropyLoss):
        raise NotImplementedError(f"{where}: the reference uses nn.CrossEntropyLoss")
    if criterion.weight is not None or getattr(criterion, "label_smoothing", 0.0) != 0.0 or criterion.reduction != "mean" or \
            criterion.ignore_index != -100:
        raise NotImplementedError(f"{where}: only the default nn.CrossEntropyLoss() (no weight / label_smoothing / ignore_index, "
                                  "reduction='mean') is implemented by the engine through the `criterion` argument; pass the options as "
                                  "args.loss_options = LossOptions.from_criterion(criterion) instead")


def _rsp_epoch(args, model, classifier, loader, criterion, optimizer, epoch, train):
    _plain_ce(criterion, "RSP pretraining (pretrain_BreastPathQ.py:56)")
    eng = get_engine(_device_of(model))
    model.train(train)
    classifier.train(train)
    net = eng.bind(model, classifier)
    meters = _meters(eng, ["loss", "acc"])
    feats, targets = [], []
    k = _micro_k(args) if train else 1
    opts = _loss_options(args)
    t0 = time.time()
    for batch_idx, (input1, input2, input3, target) in enumerate(_ahead(loader, eng, _prefetch_on(args))):
        i1, i2, i3 = (v.reshape(-1, 3, args.tile_h, args.tile_w) for v in (input1, input2, input3))
        target = target.long().view(-1, 1).reshape(-1)
        r = _sup_step(eng, net, "ce", [i1, i2, i3], target, k, opts) if train else _val_step(eng, net, [i1, i2, i3], target, opts)
        if train:
            net.optimizer_step(optimizer, max_grad_norm=getattr(args, "clip_grad_norm", None))
        meters.add(r["losses"], target.size(0))
        if train:
            feats.append(r["feats"])
            targets.append(target.to(eng.device))
        _maybe_print(args, batch_idx, "Train" if train else "Val", epoch, _len(loader), t0, meters)
    m = meters.meters()
    if train:
        return m["loss"].avg, m["acc"].avg, torch.cat(feats).detach(), torch.cat(targets).detach()
    return m["loss"].avg, m["acc"].avg


def rsp_train(args, model, classifier, train_loader, criterion, optimizer, epoch):
    """pretrain_BreastPathQ.train (= pretrain_Camelyon16, Pretraining_v2/pretrain_RSP): (loss, acc, feats, targets)."""
    return _rsp_epoch(args, model, classifier, train_loader, criterion, optimizer, epoch, True)


def rsp_validate(args, model, classifier, val_loader, criterion, epoch):
    return _rsp_epoch(args, model, classifier, val_loader, criterion, None, epoch, False)


# ------------------------------------------------------------------------------------------------ supervised fine-tune
def cam_sup_train(args, model, classifier, tumor_labeled_train_loader, normal_labeled_train_loader, optimizer, epoch):
    """eval_Camelyon_SSL.train -> (loss, acc, feats, targets)."""
    eng = get_engine(_device_of(model))
    model.train()
    classifier.train()
    net = eng.bind(model, classifier)
    meters = _meters(eng, ["loss", "acc"])
    feats, targets = [], []
    k = _micro_k(args)
    opts = _loss_options(args)
    S = args.image_size
    for batch_idx, (tumor_data_x, normal_data_x) in enumerate(_ahead(zip(tumor_labeled_train_loader, normal_labeled_train_loader), eng,
                                                                     _prefetch_on(args))):
        t_x, t_y = tumor_data_x
        n_x, n_y = normal_data_x
        t_x, t_y = t_x.reshape(-1, 3, S, S), t_y.reshape(-1)
        n_x, n_y = n_x.reshape(-1, 3, S, S), n_y.reshape(-1)
        perm = torch.randperm(2 * len(t_x))
        x, y = _cat_shuffle(t_x, n_x, perm.to(t_x.device)), _cat_shuffle(t_y, n_y, perm.to(t_y.device)).long()
        r = _sup_step(eng, net, "ce", [x], y, k, opts)
        net.optimizer_step(optimizer, max_grad_norm=getattr(args, "clip_grad_norm", None))
        meters.add(r["losses"], x.shape[0])
        feats.append(r["feats"])
        targets.append(y.to(eng.device))
    m = meters.meters()
    return m["loss"].avg, m["acc"].avg, torch.cat(feats).detach(), torch.cat(targets).detach()


def bpq_sup_train(args, model, classifier, train_loader, criterion, optimizer, epoch):
    """eval_BreastPathQ_SSL.train -> (loss, feats, targets)."""
    _loss_options(args, mse="bpq_sup_train")
    if criterion is not None and not isinstance(criterion, torch.nn.MSELoss):
        raise NotImplementedError("the reference fine-tunes BreastPathQ with nn.MSELoss")
    eng = get_engine(_device_of(model))
    model.train()
    classifier.train()
    net = eng.bind(model, classifier)
    meters = _meters(eng, ["loss"])
    feats, targets = [], []
    k = _micro_k(args)
    for batch_idx, (input1, target) in enumerate(_ahead(train_loader, eng, _prefetch_on(args))):
        x = input1.reshape(-1, 3, args.image_size, args.image_size)
        y = target.float().reshape(-1)
        r = _sup_step(eng, net, "mse", [x], y, k)
        net.optimizer_step(optimizer, max_grad_norm=getattr(args, "clip_grad_norm", None))
        meters.add(r["losses"], y.size(0))
        feats.append(r["feats"])
        targets.append(y.to(eng.device))
    m = meters.meters()
    return m["loss"].avg, torch.cat(feats).detach(), torch.cat(targets).detach()


def kather_sup_train(args, model, classifier, train_loader, criterion, optimizer, epoch):
    """eval_Kather_SSL.train (:32-99; the reference file does not parse as a whole, :243): student-only CE -> (loss, acc)."""
    _plain_ce(criterion, "Kather fine-tuning (eval_Kather_SSL.py:410)")
    eng = get_engine(_device_of(model))
    model.train()
    classifier.train()
    net = eng.bind(model, classifier)
    meters = _meters(eng, ["loss", "acc"])
    k = _micro_k(args)
    opts = _loss_options(args)
    for batch_idx, (input, target) in enumerate(_ahead(train_loader, eng, _prefetch_on(args))):
        x = input.reshape(-1, 3, args.image_size, args.image_size)                   # :57
        y = target.reshape(-1).long()
        r = _sup_step(eng, net, "ce", [x], y, k, opts)
        net.optimizer_step(optimizer, max_grad_norm=getattr(args, "clip_grad_norm", None))
        meters.add(r["losses"], y.size(0))
    m = meters.meters()
    return m["loss"].avg, m["acc"].avg


def kather_sup_validate(args, model, classifier, val_loader, criterion, epoch):
    """eval_Kather_SSL.validate (:102-151) -> (loss_avg, acc_avg): eval-mode forward + CE + accuracy."""
    _plain_ce(criterion, "Kather validation (eval_Kather_SSL.py:102-151)")
    return kather_cr_validate(args, model, classifier, val_loader, epoch)


# ------------------------------------------------------------------------------------------------ test() of the four eval scripts
_last_test = {"confusion": None, "scores": None, "targets": None, "auc": {}}


def _keep_scores(scores, targets):
    """the device tensors ``last_test_auc`` sorts when somebody asks (None: the test had no class scores)"""
    _last_test["scores"], _last_test["targets"], _last_test["auc"] = scores, targets, {}


def last_test_auc(average="macro"):
    """``sklearn.metrics.roc_auc_score(final_targets, final_pred_score, multi_class='ovr', average=average)`` of the most recent
    ``kather_cr_test`` call (eval_Kather_SSL_CR.py:658), from the scores and targets that call left on the device:
    ``inference.roc_auc`` on the first call (its launches, one copy of 4 C integers), the cached value afterwards.  The test itself
    launches and copies nothing for it.  average: 'macro', 'weighted' or None (the per-class vector).  None after a ``bpq_*_test`` or a
    test without scores (``kather_sup_test``); ``camelyon16_test`` leaves it as it was.  ``roc_auc``'s ValueErrors pass through."""
    if _last_test["scores"] is None:
        return None
    if average not in _last_test["auc"]:
        from .inference import roc_auc
        _last_test["auc"][average] = roc_auc(_last_test["scores"], _last_test["targets"], multi_class="ovr", average=average)
    return _last_test["auc"][average]


def last_test_confusion():
    """the int64 [C, C] confusion matrix (rows = targets, columns = predictions; a CPU tensor) of the most recent ``kather_cr_test`` /
    ``kather_sup_test`` call, counted on the device by sslcr_predict -- sklearn's ``confusion_matrix(final_targets,
    final_predictions, labels=range(C))`` of the returned tensors; None after a regression ``bpq_*_test``.  ``camelyon16_test`` on a
    ``WsiDeviceLoader`` that holds an annotation leaves the 2 x 2 tile-level matrix here (rows = the label of the tile's centre, columns
    = the argmax of the tile's, or the ensemble's, scores); any other ``camelyon16_test`` call leaves it as it was."""
    return _last_test["confusion"]


def _tta_codes(args):
    """args.tta: a name of ``inference.D4_SETS`` ('d4', 'rot90', 'flips') or a sequence of distinct orientation codes 0..7 -> the tuple
    of codes; absent or None = None: the code path of every earlier version, launch for launch."""
    spec = getattr(args, "tta", None)
    if spec is None:
        return None
    from .inference import d4_codes
    return d4_codes(spec)


class _Orientations:
    """the members of a host-fed batch: uploaded ONCE (``Engine.as_input``), then oriented on the device, one sslcr_d4_transform per
    listed code (code 0 is the batch itself).  Non-square inputs raise before any launch."""

    def __init__(self, eng, codes):
        self.eng, self.codes, self._table = eng, codes, None

    def members(self, input):
        from . import kernels as K
        x = input if torch.is_tensor(input) else torch.as_tensor(input)
        if x.dim() != 4 or x.shape[-1] != x.shape[-2]:
            raise ValueError(f"args.tta: square tiles [n, 3, S, S] expected, got a batch of shape {tuple(x.shape)}")
        x = self.eng.as_input(x)
        n = x.shape[0]
        if self._table is None or self._table.shape[1] < n:          # [8, n] int32, row g = g
            self._table = torch.arange(8, dtype=torch.int32).repeat_interleave(n).view(8, n).to(self.eng.device)
        for g in self.codes:
            yield x if g == 0 else K.d4_transform(x, self._table[g, :n])

    def logits(self, net, input, first_step):
        """-> ([G, n, C] logits of one batch, member g in slot g; the result of ``first_step(x)``): the FIRST listed orientation
        goes through the loop's own eval step (its loss and meters), the others through the same eval forward alone -- G passes
        over one batch layout, so every slot has the bits the plain path gives for host-oriented tiles."""
        ens = r = None
        for k, x in enumerate(self.members(input)):
            if k == 0:
                r = first_step(x)
                logits = r["logits"]
                ens = torch.empty((len(self.codes),) + tuple(logits.shape), dtype=torch.float32, device=self.eng.device)
            else:
                logits = net.forward((x,), train=False)[1]
            ens[k].copy_(logits)
        return ens, r


def _bpq_test_tta(args, net, eng, test_loader, codes):
    """``_bpq_test`` over the orientations ``codes``: ``outputs`` is the mode-1 mean of sslcr_predict_tta (the fp32 left-to-right sum of
    the members' outputs divided by float32(G)); the printed loss meter and ``feats`` are those of the FIRST listed orientation."""
    from . import kernels as K
    meters = _meters(eng, ["loss"])
    orient = _Orientations(eng, codes)
    outputs, feats, targets_a, targets_b = [], [], [], []
    t0 = time.time()
    for batch_idx, (input, targetA, targetB) in enumerate(_ahead(test_loader, eng, _prefetch_on(args))):
        targetA, targetB = targetA.float().to(eng.device), targetB.float().to(eng.device)
        ens, r = orient.logits(net, input, lambda x: eng.step_supervised(net, "mse", [x], targetA.reshape(-1), train=False))
        meters.add(r["losses"], targetA.size(0))
        feats.append(r["feats"])
        outputs.append(K.predict_tta(ens, mode=1, scores=True, pred=False)["scores"].reshape(-1))
        targets_a.append(targetA)
        targets_b.append(targetB)
        _maybe_print(args, batch_idx, "Test", 0, _len(test_loader), t0, meters)
    _last_test["confusion"] = None
    _keep_scores(None, None)
    return tuple(torch.cat(v).detach().to("cpu") for v in (outputs, feats, targets_a, targets_b))


def _bpq_test(args, model, classifier, test_loader, where):
    _loss_options(args, mse=where)
    codes = _tta_codes(args)
    eng = get_engine(_device_of(model))
    model.eval()
    classifier.eval()
    net = eng.bind(model, classifier)
    if codes is not None:
        return _bpq_test_tta(args, net, eng, test_loader, codes)
    meters = _meters(eng, ["loss"])
    outputs, feats, targets_a, targets_b = [], [], [], []
    t0 = time.time()
    for batch_idx, (input, targetA, targetB) in enumerate(_ahead(test_loader, eng, _prefetch_on(args))):
        targetA, targetB = targetA.float().to(eng.device), targetB.float().to(eng.device)
        r = eng.step_supervised(net, "mse", [input], targetA.reshape(-1), train=False)          # F.mse_loss(output, targetA.view(-1, 1))
        meters.add(r["losses"], targetA.size(0))
        outputs.append(r["logits"].reshape(-1))
        feats.append(r["feats"])
        targets_a.append(targetA)
        targets_b.append(targetB)
        _maybe_print(args, batch_idx, "Test", 0, _len(test_loader), t0, meters)
    _last_test["confusion"] = None
    _keep_scores(None, None)
    return tuple(torch.cat(v).detach().to("cpu") for v in (outputs, feats, targets_a, targets_b))


def bpq_test(args, model_student, classifier_student, test_loader):
    """eval_BreastPathQ_SSL_CR.test (:178-242) -> (outputs [n], feats [n, 768], targetsA, targetsB) on the CPU.

    ``args.tta`` (see ``camelyon16_test``): ``outputs`` is the mean of the regression outputs over the listed orientations (mode 1
    of sslcr_predict_tta).  The printed loss meter and ``feats`` are those of the FIRST listed orientation: features are not averaged."""
    return _bpq_test(args, model_student, classifier_student, test_loader, "bpq_test")


def bpq_sup_test(args, model, classifier, criterion, test_loader):
    """eval_BreastPathQ_SSL.test (:152-216; ``criterion`` before the loader, as there) -> (outputs, feats, targetsA, targetsB).
    ``args.tta``: as ``bpq_test`` (mean outputs; loss meter and ``feats`` of the first listed orientation)."""
    if criterion is not None and not isinstance(criterion, torch.nn.MSELoss):
        raise NotImplementedError("the reference tests BreastPathQ with nn.MSELoss")
    return _bpq_test(args, model, classifier, test_loader, "bpq_sup_test")


def _cls_test(args, model, classifier, test_loader, want_scores):
    from . import kernels as K
    codes = _tta_codes(args)
    eng = get_engine(_device_of(model))
    model.eval()
    classifier.eval()
    net = eng.bind(model, classifier)
    meters = _meters(eng, ["loss", "acc"])
    opts = _loss_options(args)
    confusion = torch.zeros((net.ncls, net.ncls), dtype=torch.int64, device=eng.device)
    orient = _Orientations(eng, codes) if codes is not None else None
    preds, targets, scores = [], [], []
    t0 = time.time()
    for batch_idx, (input, target) in enumerate(_ahead(test_loader, eng, _prefetch_on(args))):
        target = target.long().reshape(-1).to(eng.device).contiguous()
        if orient is not None:
            ens, r = orient.logits(net, input, lambda x: _val_step(eng, net, [x], target, opts))
            meters.add(r["losses"], target.size(0))
            p = K.predict_tta(ens, target, scores=want_scores, pred=True, confusion=confusion)
        else:
            r = _val_step(eng, net, [input], target, opts)
            meters.add(r["losses"], target.size(0))
            p = K.predict(r["logits"], target, scores=want_scores, pred=True, confusion=confusion)
        preds.append(p["pred"])
        targets.append(target)
        if want_scores:
            scores.append(p["scores"])
        _maybe_print(args, batch_idx, "Test", 0, _len(test_loader), t0, meters)
    all_targets = torch.cat(targets)
    out = [torch.cat(preds).to("cpu"), all_targets.to("cpu")]
    if want_scores:
        all_scores = torch.cat(scores)
        out.append(all_scores.to("cpu"))
    _last_test["confusion"] = confusion.to("cpu")
    _keep_scores(all_scores if want_scores else None, all_targets if want_scores else None)    # references, for last_test_auc()
    return tuple(out)


def kather_cr_test(args, model, classifier, test_loader):
    """eval_Kather_SSL_CR.test (:182-245) -> (predictions int64 [n], targets int64 [n], pred_score [n, 9]) on the CPU.

    ``args.tta`` (see ``camelyon16_test``): ``pred_score`` is the mean softmax over the listed orientations, ``predictions`` its
    argmax (lowest index), and ``last_test_confusion()`` counts those predictions, once per image.  The printed loss and accuracy
    meters are those of the FIRST listed orientation."""
    return _cls_test(args, model, classifier, test_loader, True)


def kather_sup_test(args, model, classifier, test_loader, criterion):
    """eval_Kather_SSL.test (:154-213; ``criterion`` last, as there) -> (predictions, targets).  ``args.tta``: as ``kather_cr_test``
    (ensemble predictions; the meters are the first listed orientation's)."""
    _plain_ce(criterion, "Kather test (eval_Kather_SSL.py:154-213)")
    return _cls_test(args, model, classifier, test_loader, False)


# ------------------------------------------------------------------------------------------------ WSI inference (f3)
def _camelyon16_test_device(args, net, loader, codes=None):
    """the device-resident loader: per batch a tile gather, the eval forward and the softmax column scattered into the map, all on
    the current stream; no host sync and no device-to-host copy before the one copy of the finished map.  codes (args.tta): per
    batch and per listed orientation one oriented gather (sslcr_wsi_gather_d4) and one eval forward into slot g of a [G, n, C]
    logits buffer, then ONE sslcr_predict_tta into the map -- still no sync, still one copy."""
    import numpy as np
    from . import kernels as K
    mask = loader.dataset.mask
    probs = torch.zeros(mask.shape, dtype=torch.float32, device=loader.region.device)
    # a loader with an annotation: the same launch also counts confusion[label of the tile's centre][argmax], every tile once
    targets = getattr(loader, "targets", None)
    counted = {}
    if targets is not None:
        counted["confusion"] = torch.zeros((net.ncls, net.ncls), dtype=torch.int64, device=loader.region.device)
    t0 = time.time()
    for batch_idx, (lo, hi) in enumerate(loader.ranges()):
        if targets is not None:
            counted["target"] = targets[lo:hi]
        if codes is not None:
            ens = torch.empty((len(codes), hi - lo, net.ncls), dtype=torch.float32, device=loader.region.device)
            for k, g in enumerate(codes):
                ens[k].copy_(net.forward((loader.tiles(lo, hi, orient=g),), train=False)[1])
            K.predict_tta(ens, pred=False, col=-1, map=probs, map_index=loader.map_index[lo:hi], **counted)
        else:
            _, output = net.forward((loader.tiles(lo, hi),), train=False)
            K.predict(output, pred=False, col=-1, map=probs, map_index=loader.map_index[lo:hi], **counted)   # second column 'tumor' (:58-62)
        if (batch_idx + 1) % 10 == 0 and getattr(args, "print_freq", 0):
            print("Test: [{0}/{1}]\tBT {2:.3f} (enqueue)".format(batch_idx, len(loader), (time.time() - t0) / (batch_idx + 1)))
    out = probs.cpu().numpy().astype(np.float64)
    if targets is not None:
        _last_test["confusion"] = counted["confusion"].to("cpu")
    return out


def camelyon16_test(args, model, classifier, test_loader):
    """test_Camelyon16.test (test_Camelyon16.py:30-70) -> probs_map: every tissue pixel of ``test_loader.dataset.mask``
    gets the softmax 'tumor' probability of its tile; forward-only (BatchNorm folded, all epilogues fused).  An
    ``inference.WsiDeviceLoader`` is served from the slide bytes it holds in HBM (same map, no per-batch host traffic); one built with
    ``annotation=`` also has the launch count the tile-level confusion matrix against the annotation's labels (``last_test_confusion()``).

    ``args.tta`` (a name of ``inference.D4_SETS`` or a sequence of orientation codes; absent or None = off): every tile is scored
    under each listed flip / quarter turn and the map holds the mean 'tumor' probability -- the fp32 sum of the members in the order
    listed, divided by float32(G) (sslcr_predict_tta).  Square tiles only; a host-fed batch is uploaded once and oriented on the
    device."""
    import numpy as np
    from . import kernels as K
    from .inference import WsiDeviceLoader
    codes = _tta_codes(args)
    eng = get_engine(_device_of(model))
    model.eval()
    classifier.eval()
    net = eng.bind(model, classifier)
    if isinstance(test_loader, WsiDeviceLoader):
        return _camelyon16_test_device(args, net, test_loader, codes)
    orient = _Orientations(eng, codes) if codes is not None else None
    probs_map = np.zeros(test_loader.dataset.mask.shape)
    t0 = time.time()
    for batch_idx, (input, x_mask, y_mask) in enumerate(_ahead(test_loader, eng, _prefetch_on(args))):
        if orient is not None:
            ens, _ = orient.logits(net, input, lambda x: dict(logits=net.forward((x,), train=False)[1]))
            probs = K.predict_tta(ens, scores=True, pred=False)["scores"][:, -1].cpu().numpy()
        else:
            _, output = net.forward((input,), train=False)
            probs = K.softmax_col(output.contiguous(), -1).cpu().numpy()    # second column 'tumor' (:58-60)
        probs_map[x_mask.numpy(), y_mask.numpy()] = probs
        if (batch_idx + 1) % 10 == 0 and getattr(args, "print_freq", 0):
            print("Test: [{0}/{1}]\tBT {2:.3f}".format(batch_idx, _len(test_loader), (time.time() - t0) / (batch_idx + 1)))
    return probs_map


def teacher_refresh(model_teacher, classifier_teacher, model_student, classifier_student, ema_decay=0.0):
    """In-place form of the reference's per-epoch ``teacher = copy.deepcopy(student)`` (eval_BreastPathQ_SSL_CR.py:515-516),
    generalised to an EMA (decay 0 == the reference).  ``copy.deepcopy`` itself also works on these modules."""
    eng = get_engine(_device_of(model_student))
    te, st = eng.bind(model_teacher, classifier_teacher), eng.bind(model_student, classifier_student)
    te.ema_from(st, ema_decay)


# ------------------------------------------------------------------------------------------------ k-NN feature probe
def _probe_features(args, eng, net, loader):
    """the eval forward ``*_validate`` runs (``BoundNet.forward(train=False)``; one tile, or the three RSP tiles) over a loader of
    ``(*tiles, target)`` batches: -> (feats [n, 768], targets [n]) gathered on the device"""
    feats, targets = [], []
    for batch in _ahead(loader, eng, _prefetch_on(args)):
        *tiles, target = batch
        xs = [v.reshape(-1, *v.shape[-3:]) for v in tiles]
        f, _ = net.forward(xs, train=False)
        feats.append(f)
        targets.append(target.reshape(-1).to(eng.device))
    return torch.cat(feats), torch.cat(targets)


def knn_probe(args, model, classifier, bank_loader, query_loader=None, k=20, **kw):
    """The k-NN probe of the features a (model, classifier) pair computes: leave-one-out over ``bank_loader`` when there is no
    ``query_loader``, else the bank's labels voted onto the queries.  Integer targets -> ``inference.knn_probe``'s dict
    (``accuracy``, ``confusion``, ``pred``, ...); float targets (BreastPathQ) -> dict with ``pred`` and ``mse``, the k-NN regressor's
    predictions (leave-one-out or on the queries) and their mean squared error.  Features and targets stay on the device; one copy of
    the final numbers: the class count is the classifier's own (``n_classes=`` overrides it), nothing is read off the labels.  Keywords:
    ``inference.knn_probe``'s (``metric``, ``weights``, ``temperature``, ``n_classes``) for integer targets, ``metric`` alone for float
    targets; any other raises."""
    from . import inference as I
    eng = get_engine(_device_of(model))
    model.eval()
    classifier.eval()
    net = eng.bind(model, classifier)
    feats, targets = _probe_features(args, eng, net, bank_loader)
    q = qt = None
    if query_loader is not None:
        q, qt = _probe_features(args, eng, net, query_loader)
    if not targets.is_floating_point():
        kw.setdefault("n_classes", net.ncls)
        return I.knn_probe(feats, targets, k, query_loader is None, queries=q, query_targets=qt, **kw)
    metric = kw.pop("metric", "cosine")
    if kw:
        raise TypeError(f"knn_probe: {sorted(kw)} do not apply to float targets (the k-NN regressor takes metric only)")
    bank = I.FeatureBank(feats.shape[1], metric=metric).add(feats, targets).finalize()
    r = I.knn_regress(bank, q, k, exclude_self=0 if q is None else None)
    truth = (targets if qt is None else qt).float()
    flat = torch.cat([r["pred"], ((r["pred"] - truth) ** 2).mean().reshape(1)]).cpu().numpy()
    return dict(pred=flat[:-1], mse=float(flat[-1]))


def linear_probe(args, model, classifier, train_loader, test_loader=None, *, sample_weight=None, **kw):
    """The linear probe of the features a (model, classifier) pair computes -- the reference's ``--modules 64`` ("fine-tune only
    classifier") solved as the convex problem it is: the eval forward runs ONCE over ``train_loader`` (and ``test_loader``), then
    ``inference.linear_probe`` fits the head on the device-resident features.  Integer targets -> ``accuracy``, ``confusion``,
    ``pred``, ... (on ``test_loader`` when given, else the training figures); float targets (BreastPathQ) -> ``pred`` and ``mse``; plus
    ``probe``, whose ``to_classifier(classifier)`` installs the fitted head.  The class count is the classifier's own (``n_classes=``
    overrides it), nothing is read off the labels.  Deviation: the probe sees the EVAL forward's features (BatchNorm on running
    statistics); the reference's frozen mode calls ``model.train()`` and so runs BatchNorm on batch statistics.  sample_weight: one
    weight per row of ``train_loader`` in its order (device float32), passed to the fit.  kw: ``inference.LinearProbe``'s."""
    from . import inference as I
    eng = get_engine(_device_of(model))
    model.eval()
    classifier.eval()
    net = eng.bind(model, classifier)
    feats, targets = _probe_features(args, eng, net, train_loader)
    q = qt = None
    if test_loader is not None:
        q, qt = _probe_features(args, eng, net, test_loader)
    if not targets.is_floating_point():
        kw.setdefault("n_classes", net.ncls)
    return I.linear_probe(feats, targets, queries=q, query_targets=qt, sample_weight=sample_weight, **kw)

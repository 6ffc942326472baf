"""MI355X execution engine for the ResNet family: the whole network body (stem + all residual
blocks) is ONE autograd node whose forward and backward are explicit sequences of the
hand-written HIP kernels.

Why one node: the reference runs ~7 kernels and 3-4 activation passes per FusedConvBN in
forward and ~15 in backward, recomputing the conv (resnet.py:72-113, survey CS4).  Here
each convolution is one implicit-GEMM MFMA kernel whose prologue applies the producer's
batch-norm + activation while staging the operand (a conv output is never normalised in
memory) and whose epilogue emits the per-channel statistics of its own output.  Backward
is likewise one dgrad kernel (prologue: the batch-norm backward correction
g + alpha + beta*y; epilogue: the consumer activation backward + the producer's
statistics reductions) and one wgrad kernel per convolution.  Owning the whole body lets
the engine

* accumulate the two data-gradient contributions of a block input (residual path and
  shortcut) inside the second dgrad's epilogue (no autograd sum kernel),
* write weight / BN-affine gradients straight into the flat gradient buffer and signal
  DDP bucket readiness itself (``grad_ready``), in backward order,
* pack every conv weight to bf16 GEMM layouts in one launch per step,
* stay free of host synchronisation and allocation-order dependence, so a whole train
  step can be captured in a HIP graph.

Numerics follow the reference exactly where it defines the model: FusedConvBN uses batch
statistics in train AND eval with unbiased variance and (y-mean)/(sqrt(var)+1e-3)
(resnet.py:75-100); nn.BatchNorm2d uses biased variance, affine, running statistics with
momentum (resnet.py:204-206, 221-223).  Compute is bf16 MFMA with fp32 accumulation and
fp32/fp64 statistics.
"""
from __future__ import annotations

import os
import struct
from collections import OrderedDict

import torch
import torch.nn as nn

from . import _native
from . import conv_igemm as ci
from ..parallel import graphs as _graphs

ACT_NONE, ACT_RELU, ACT_CELU = 0, 1, 2
# materialise the normalised input / folded gradient of 3x3 convs once (see forward/backward)
MATERIALIZE_3X3 = os.environ.get("FDT_MATERIALIZE_3X3", "1") != "0"
# run a block's ReLU join inside the next block's first 1x1 conv (PRO_JOIN prologue) instead
# of a standalone pass (see ResNetBodyFn.forward)
JOIN_FOLD = os.environ.get("FDT_JOIN_FOLD", "1") != "0"
# widest next-block 1x1 (output channels) that still takes the join fold (_join_fold_tile: one
# output-channel tile, and 256 only at >= 65536 rows)
JOIN_FOLD_MAX = int(os.environ.get("FDT_JOIN_FOLD_MAX", "256"))
# ... and, past 64 output channels without a tuned "fwd3" entry, only over at least this many rows
# (batch 128's stage-2 joins measured 0.2 % slower folded: profiles/r5/joinfold_bs128_*.json)
JOIN_FOLD_MIN_M = int(os.environ.get("FDT_JOIN_FOLD_MIN_M", str(1 << 18)))
# run the classifier head (average pool + fc, bf16 autocast numerics) as two engine kernels
# inside the body's graphs instead of eager PyTorch ops (see csrc/kernels/head.hip)
FUSED_HEAD = os.environ.get("FDT_FUSED_HEAD", "1") != "0"
HEAD_MAX_CLASSES = 256  # head.hip's cap (CIFAR-100, Tiny-ImageNet's 200); wider heads run as PyTorch ops
MODE_FCBN, MODE_BN_TRAIN, MODE_BN_EVAL, MODE_FCBN_TRACK = 0, 1, 2, 3
BF16 = torch.bfloat16

# Parameters whose gradient the engine writes itself call these hooks (the DDP reducer
# registers here in addition to autograd's post-accumulate-grad hooks).  A "deferrable"
# hook (the reducer's) takes ``defer=True`` and returns its GPU action (a bucket
# all-reduce) instead of launching it, so that, while capturing, the HIP graph can be cut
# there.
_GRAD_READY_HOOKS: dict[int, list] = {}


def register_grad_ready_hook(param, fn, deferrable=False):
    ent = (fn, bool(deferrable))
    _GRAD_READY_HOOKS.setdefault(id(param), []).append(ent)

    class _Handle:
        def remove(self_inner):
            lst = _GRAD_READY_HOOKS.get(id(param), [])
            if ent in lst:
                lst.remove(ent)
    return _Handle()


# While a backward is being captured into HIP graphs (parallel/graphs.py recording),
# deferrable hooks return their GPU action; the recorder cuts the graph there so the action
# runs between two graph segments on every replay (communication keeps overlapping backward).
def grad_ready(param):
    hooks = _GRAD_READY_HOOKS.get(id(param), ())
    if not hooks:
        return
    rec = _graphs.active()
    acts = []
    for fn, deferrable in hooks:
        if deferrable:
            a = fn(param, defer=True)
            if a is not None:
                acts.append(a)
        else:
            fn(param)
    if not acts:
        return
    if rec is not None:
        rec.cut(acts)
    else:
        for a in acts:
            a()


def _sp():
    return _native.stream_ptr()


def _p(t):
    return 0 if t is None else t.data_ptr()


def _f32(n, dev):
    return torch.empty(n, device=dev, dtype=torch.float32)


class Unit:
    """One convolution + its normalisation."""

    def __init__(self, conv, bn, act_out):
        from ..models.resnet import FusedConvBN
        if isinstance(conv, FusedConvBN):
            self.w = conv.conv_weight
            stride, pad = 1, conv.padding
            self.bn = None
            self.fc = conv  # (tracked running statistics: models.resnet.enable_running_stats)
            self.eps = conv.eps
        else:
            assert isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d)
            self.w = conv.weight
            stride, pad = conv.stride[0], conv.padding[0]
            self.bn = bn
            self.fc = None
            self.eps = bn.eps
        cout, cin, k, _ = self.w.shape
        self.shp = ci.ConvShape(cin, cout, k, stride, pad)
        self.act_out = act_out  # activation the consumer applies to this unit's normalised output
        self.wf = self.wd = None

    def mode(self, training):
        if self.bn is None:
            return MODE_FCBN_TRACK if (training and self.fc.track_running_stats) else MODE_FCBN
        use_batch = training or not self.bn.track_running_stats
        return MODE_BN_TRAIN if use_batch else MODE_BN_EVAL

    def ensure_packed_buffers(self, dev, need_dgrad):
        need_wd = need_dgrad and self.shp.cin >= 8
        if self.wf is None or self.wf.device != dev:
            self.wf, self.wd = ci.alloc_packed(self.shp, dev, dgrad=need_wd)
        elif need_wd and self.wd is None:
            # (an eval / no-grad forward packs no dgrad layout; a later train step needs it)
            self.wd = ci.alloc_packed(self.shp, dev, dgrad=True, fwd=False)[1]


def _act_of(m):
    if isinstance(m, nn.ReLU):
        return (ACT_RELU, 1.0)
    if isinstance(m, nn.CELU):
        return (ACT_CELU, float(m.alpha))
    return None


def _chain(seq: nn.Sequential):
    """nn.Sequential of (FusedConvBN | Conv2d+BatchNorm2d | activation) -> [Unit]."""
    mods = list(seq)
    units = []
    i = 0
    while i < len(mods):
        m = mods[i]
        a = _act_of(m)
        if a is not None:
            assert units, "activation before any conv"
            units[-1].act_out = a
            i += 1
            continue
        if isinstance(m, nn.Conv2d):
            units.append(Unit(m, mods[i + 1], (ACT_NONE, 1.0)))
            i += 2
        else:
            units.append(Unit(m, None, (ACT_NONE, 1.0)))
            i += 1
    return units


class Block:
    def __init__(self, blk):
        from ..models.resnet import BottleNeck
        self.units = _chain(blk.residual_function)
        sc = _chain(blk.shortcut) if len(blk.shortcut) > 0 else []
        assert len(sc) <= 1
        self.shortcut = sc[0] if sc else None
        self.join = (ACT_RELU, 1.0) if isinstance(blk, BottleNeck) else (ACT_CELU, 0.075)


STAGES = ("conv2_x", "conv3_x", "conv4_x", "conv5_x")

# The flat optimizer writes the packed conv weight layouts itself (optim_pack.hip: one fused
# update-and-pack launch) when the model's weights live in its flat buffer; the forward then
# skips its repack while nothing else has written the weights since (Plan.pack_fresh)
PACK_IN_OPT = os.environ.get("FDT_PACK_IN_OPT", "0") == "1"


class Plan:
    def __init__(self, model):
        stem_seq = model.conv1
        self.stem = Unit(stem_seq[0], None, _act_of(stem_seq[1]))
        self.blocks, self.stage_of = [], []
        for name in STAGES:
            for b in getattr(model, name):
                self.blocks.append(Block(b))
                self.stage_of.append(name)
        self.units = [self.stem] + [u for b in self.blocks for u in (b.units + ([b.shortcut] if b.shortcut else []))]
        self.fsdp = None  # parallel/fsdp.py FullyShardedDP driving the stages as wrap units

    def tracking(self):
        """The momenta of the FusedConvBN units that update running statistics in train-mode
        forwards (None: cumulative), in plan order; empty (false) when none does."""
        return tuple(u.fc.momentum for u in self.units if u.fc is not None and u.fc.track_running_stats)

    def pack(self, dev, need_dgrad=True):
        if self.pack_fresh():
            return  # the optimizer's fused step already wrote both layouts from these weights
        ents = []
        for u in self.units:
            had = (u.wf, u.wd)
            u.ensure_packed_buffers(dev, need_dgrad and u is not self.stem)
            if u.wf is not had[0] or u.wd is not had[1]:
                self.__dict__.pop("_upd", None)  # the optimizer's table points at the old buffers
            ents.append((u.w.detach(), u.wf, u.wd, u.shp))
        ci.pack_weights(ents)

    # ---- packed layouts written by the optimizer (optim_pack.hip)
    def _weights_version(self, flat):
        # torch in-place writes (load_state_dict, copy_ into the flat buffer or a parameter) bump
        # these counters; the native optimizer kernels do not
        return flat.data._version + sum(u.w._version for u in self.units)

    def update_table(self, flat):
        """Launches of the fused update-and-pack step over ``flat`` (a FlatParams holding every
        conv weight as a contiguous fp32 OIHW view): a list of (entries int64 [n, 8], n, conv
        blocks, rest ranges int64 [m, 3], m, rest elements, max taps, counts a skipped step) --
        the 1x1 weights with every non-conv range at a 4 KB LDS image, then the 3x3 / 2x2
        weights at 38 KB -- or None when the layouts are not allocated yet (before the first
        training forward) or the weights are not all in ``flat``."""
        if not PACK_IN_OPT or self.fsdp is not None or not flat.data.is_cuda:
            return None
        c = self.__dict__.get("_upd")
        if c is not None and c[0] is flat:
            return c[1]
        if any(u.wf is None or (u.wd is None and u.shp.cin >= 8) for u in self.units):
            return None
        base, n = flat.data.data_ptr(), flat.numel
        rows = {1: [], 9: []}
        blks = {1: 0, 9: 0}
        spans = []
        for u in self.units:
            w = u.w
            off, rem = divmod(w.data_ptr() - base, 4)
            if (w.dtype != torch.float32 or not w.is_contiguous() or rem or off < 0 or off + w.numel() > n
                    or w.device != flat.data.device or w.dim() != 4):
                return None
            co, cin, kh, kw = w.shape
            if kh * kw not in (1, 4, 9) or co % 8 or u.shp.cxp % 8 or u.wf.device != w.device:
                return None
            g = 1 if kh * kw == 1 else 9
            rows[g].append([off, u.wf.data_ptr(), 0 if u.wd is None else u.wd.data_ptr(), co, cin, u.shp.cxp,
                            kh * kw, blks[g]])
            blks[g] += -(-co // 32) * -(-u.shp.cxp // 64)
            spans.append((off, off + w.numel()))
        spans.sort()
        rr, cur, cum = [], 0, 0
        for a, b in spans:
            if a < cur:
                return None  # overlapping weights
            if a > cur:
                rr.append([cur, a - cur, cum])
                cum += a - cur
            cur = b
        if cur < n:
            rr.append([cur, n - cur, cum])
            cum += n - cur
        dev = flat.data.device
        keep, launches = [], []
        for g in (1, 9):
            with_rest = g == 1
            if not rows[g] and not (with_rest and cum):
                continue
            tab = torch.tensor(rows[g] or [[0] * 8], dtype=torch.int64, device=dev)
            rrt = torch.tensor(rr or [[0, 0, 0]], dtype=torch.int64, device=dev)
            keep += [tab, rrt]
            launches.append((tab.data_ptr() if rows[g] else 0, len(rows[g]), blks[g],
                             rrt.data_ptr() if with_rest and rr else 0, len(rr) if with_rest else 0,
                             cum if with_rest else 0, g, int(not launches)))
        self._upd = (flat, launches, keep)
        # generation of the table: an NGD graph captured with the fused repack baked in the
        # table / layout addresses keys on it (optim/ngd.py _graph_key) -- a rebuilt table (new
        # packed buffers) never replays a graph holding the old, freed ones
        self.upd_gen = getattr(self, "upd_gen", 0) + 1
        return launches

    def mark_opt_packed(self, flat):
        """The optimizer step just written (or, when skipped on the device, left unchanged) the
        weights together with both packed layouts."""
        self._pk = (flat, self._weights_version(flat))

    def invalidate_pack(self):
        self.__dict__.pop("_pk", None)

    def pack_fresh(self) -> bool:
        pk = self.__dict__.get("_pk")
        return pk is not None and pk[1] == self._weights_version(pk[0])

    # ---- FSDP: units are gathered stage by stage, so weights are packed per stage (the
    # forward layout before the stage's forward, the dgrad layout before its backward) and
    # the packed copies are released with the gathered parameters
    def stage_units(self, name):
        if name == "conv1":
            return [self.stem]
        return [u for b, st in zip(self.blocks, self.stage_of) if st == name
                for u in (b.units + ([b.shortcut] if b.shortcut else []))]

    def pack_stage(self, name, dev, fwd: bool):
        ents = []
        for u in self.stage_units(name):
            need_wd = (not fwd) and u is not self.stem
            u.ensure_packed_buffers(dev, need_wd)
            _restore(u.wf if fwd else u.wd)
            if fwd or need_wd:
                ents.append((u.w.detach(), u.wf if fwd else None, None if fwd else u.wd, u.shp))
        ci.pack_weights(ents)

    def release_stage(self, name, fwd: bool):
        if self.fsdp is not None and self.fsdp.static:
            return  # static FSDP (graphs): packed layouts keep their addresses
        for u in self.stage_units(name):
            _release(u.wf if fwd else u.wd)


def _release(t):
    if t is not None and t.untyped_storage().size() != 0:
        t.untyped_storage().resize_(0)


def _restore(t):
    if t is not None and t.untyped_storage().size() == 0:
        t.untyped_storage().resize_(t.numel() * t.element_size())


# ------------------------------------------------------------------ kernels glue
_SLOTS: dict = {}


def slots(nq, C, dev, M):
    """The persistent statistics-slot workspace viewed as [rows, nq, C] for a producer over
    M output rows (rows = 64, or one per workgroup in deterministic mode: ci.slot_rows).
    Producers (conv epilogues, BN-backward reductions) add into it with fp32 atomics; the
    consuming finalize / reduce kernel sums it in fp64 and re-zeroes it, so the next
    producer needs no memset.  One workspace suffices: every producer is consumed before
    the next one (and a view only ever covers rows its finalize re-zeroes)."""
    rows = ci.slot_rows(M)
    n = max(ci.STAT_SLOTS * 3 * 2048, rows * nq * C)
    ws = _SLOTS.get(dev)
    if ws is None or ws.numel() < n:
        # (allocation happens in the eager warm-up step, before any graph capture)
        ws = torch.zeros(n, device=dev, dtype=torch.float32)
        _SLOTS[dev] = ws
    return ws[: rows * nq * C].view(rows, nq, C)


def _bn_fin_params(u: Unit, training):
    bn = u.bn
    mode = u.mode(training)
    if bn is not None:
        mom = bn.momentum if bn.momentum is not None else -1.0  # (None: cumulative average, bn_math.h)
        track = training and bn.track_running_stats
        rm = bn.running_mean if (track or mode == MODE_BN_EVAL) else None
        rv = bn.running_var if (track or mode == MODE_BN_EVAL) else None
        nbt = bn.num_batches_tracked if track else None
        return mode, mom, rm, rv, nbt, bn.weight, bn.bias
    if mode == MODE_FCBN_TRACK:
        fc = u.fc
        mom = fc.momentum if fc.momentum is not None else -1.0
        return mode, mom, fc.running_mean, fc.running_var, fc.num_batches_tracked, None, None
    return mode, 0.0, None, None, None, None, None


def conv_bn_fwd(x, u: Unit, s, t, act, training, dev):
    """One unit's conv + batch statistics -> (y, (s, t, save_mean, save_aux), M)."""
    Ho, Wo = ci.out_hw(x.shape[1], x.shape[2], u.shp)
    M = x.shape[0] * Ho * Wo
    st, fin = _fin_args(u, M, training, dev)
    y, _ = ci.conv_fwd(x, u.wf, u.shp, s, t, act[0] if act else 0, act[1] if act else 1.0,
                       part=slots(2, u.shp.cout, dev, M), fin=fin)
    return y, st, M


def conv_bn_fwd_join(pj, u: Unit, training, dev, tile=None):
    """``conv_bn_fwd`` of a block's first (1x1) unit whose input is the PREVIOUS block's
    join, computed in the conv's operand staging (ci.conv_fwd_join); the join output (this
    block's x_in) and its ReLU mask are stored on the way.  pj = (y, s, t, r, s2, t2, out,
    mask); ``tile``: _join_fold_tile's choice (None / "tuned": the tuned table)."""
    y, s, t, r, s2, t2, out, mask = pj
    M = y.numel() // y.shape[-1]
    st, fin = _fin_args(u, M, training, dev)
    tile = None if tile == "tuned" else tile
    yo, _ = ci.conv_fwd_join(y, r, s, t, s2, t2, u.wf, u.shp, out, mask, part=slots(2, u.shp.cout, dev, M), fin=fin,
                             tile=tile)
    return yo, st, M


def _join_fold_tile(b_next, shape):
    """Tile of the next block's first 1x1 conv when it computes this block's join in its operand
    staging (PRO_JOIN), or None for a standalone join pass.  The fused kernel wins when ONE
    output-channel tile covers the conv (each joined row is then computed and stored once;
    with several column tiles every tile re-reads both join operands: 1.2-2x slower than
    conv + join pass) -- scripts/join_probe.py, profiles/r5/join_probe_*.txt:
      Cout 64  (stage 1): the tuned tile; batch 1024 475 -> 355 us, batch 128 50 -> 44 us
      Cout 128 (stage 2): 128x128x64 at >= 2^17 rows (242 -> 195 us), else 64x128x64 (31 -> 25 us
                          in isolation, yet the batch-128 step measured 0.2 % slower folded)
      Cout 256 (stage 3): 128x256x64 at >= 2^16 rows (133 -> 124 us); slower at batch 128.
    A shape with a conv_tuned.json "fwd3" entry (scripts/retune_graph.py) is folded at that
    entry ("tuned"); others past 64 channels only over >= JOIN_FOLD_MIN_M rows.  Whole step at
    batch 1024: 25.66 -> 25.33 ms (profiles/r5/joinfold_bs1024_*.json).  ``shape``: the join's
    NHWC shape."""
    u = b_next.units[0]
    N, H = int(shape[0]), int(shape[1])
    M = N * H * int(shape[2])
    if not (JOIN_FOLD and u.shp.k == 1 and u.shp.stride == 1 and u.shp.pad == 0 and u.shp.cin == u.shp.cxp
            and u.shp.cin >= 8 and u.shp.cout <= JOIN_FOLD_MAX):
        return None
    if u.shp.cout <= 64:
        return "tuned"
    if u.shp.cout > 256 or (u.shp.cout > 128 and M < (1 << 16)):
        return None
    if ci.tuned("fwd3", N, H, u.shp):
        return "tuned"
    if M < JOIN_FOLD_MIN_M:
        return None
    if u.shp.cout <= 128:
        return (128, 128, 64) if M >= (1 << 17) else (64, 128, 64)
    return (128, 256, 64)


def _fin_args(u: Unit, M, training, dev):
    """Outputs (s, t, save_mean, save_aux) and the finalisation arguments of one unit's
    statistics (eval-mode BN reads none of them but still re-zeroes the slots)."""
    C = u.shp.cout
    s, t, sm, sa = _f32(C, dev), _f32(C, dev), _f32(C, dev), _f32(C, dev)
    mode, mom, rm, rv, nbt, gamma, beta = _bn_fin_params(u, training)
    fptr = [_p(gamma), _p(beta), _p(rm), _p(rv), _p(nbt), s.data_ptr(), t.data_ptr(), sm.data_ptr(), sa.data_ptr()]
    return (s, t, sm, sa), (fptr, [float(mode), float(u.eps), float(mom), float(M)])


def reduce_parts(part, nq, C, dev):
    nat = _native.native()
    out = torch.empty(nq, C, device=dev, dtype=torch.float32)
    nat.reduce_partials(part.data_ptr(), part.shape[0], nq, C, out.data_ptr(), 1, _sp())
    return out


def _coef_args(u: Unit, sm, sa, M, training, dev):
    """Kernel arguments of one unit's BN-backward coefficients; allocates (alpha, beta)
    and the BN affine gradients (accumulated into the flat gradient buffer)."""
    C = u.shp.cout
    al, be = _f32(C, dev), _f32(C, dev)
    gamma = u.bn.weight if u.bn is not None else None
    gg = gb = None
    if u.bn is not None:
        for p in (u.bn.weight, u.bn.bias):
            if p.requires_grad and p.grad is None:
                p.grad = torch.zeros_like(p)
        gg = u.bn.weight.grad if u.bn.weight.requires_grad else None
        gb = u.bn.bias.grad if u.bn.bias.requires_grad else None
    mode = u.mode(training)
    if mode == MODE_FCBN_TRACK:
        mode = MODE_FCBN  # the backward of a tracked unit is the untracked one's (same saved statistics)
    args = [mode, float(u.eps), float(M), sm.data_ptr(), sa.data_ptr(), _p(gamma), al.data_ptr(),
            be.data_ptr(), _p(gg), _p(gb)]
    return args, (al, be)


_NO_UNIT = [0, 0.0, 1.0, 0, 0, 0, 0, 0, 0, 0]


def coef_args(ua, sta, ub=None, stb=None, training=True, dev=None):
    """BN-backward coefficient arguments of unit ``ua`` (rows (0, 1) of the dL/dy slots) and,
    with nq == 3, of the block's shortcut unit ``ub`` (rows (2, 1)); ``st*`` = (save_mean,
    save_aux, M).  Returns ((fptr, fval) for ci.conv_dgrad(coef=...) / the standalone
    kernel, (alpha_a, beta_a), (alpha_b, beta_b) or None)."""
    aa, ra = _coef_args(ua, sta[0], sta[1], sta[2], training, dev)
    if ub is not None:
        ab, rb = _coef_args(ub, stb[0], stb[1], stb[2], training, dev)
    else:
        ab, rb = _NO_UNIT, None
    fptr = list(aa[3:]) + list(ab[3:])
    fval = [float(aa[0]), float(aa[1]), float(aa[2]), float(ab[0]), float(ab[1]), float(ab[2])]
    return (fptr, fval), ra, rb


def coef_ready(*units):
    for u in units:
        if u is not None and u.bn is not None:
            grad_ready(u.bn.weight)
            grad_ready(u.bn.bias)


def bwd_finalize(part, nq, ua, sta, ub=None, stb=None, training=True, dev=None):
    """Statistics slots [S, nq, C] of dL/dy reductions -> BN-backward corrections in one
    standalone launch (the slots are re-zeroed).  Returns ((alpha_a, beta_a), (alpha_b,
    beta_b) or None)."""
    (fptr, fval), ra, rb = coef_args(ua, sta, ub, stb, training, dev)
    ci._finalize_standalone(_native.native(), 2, part, nq, ua.shp.cout, fptr, fval)
    coef_ready(ua, ub)
    return ra, rb


def wgrad_into(u: Unit, g, y, al, be, x, xs, xt, act, gs=None):
    if u.w.grad is None:
        u.w.grad = torch.zeros_like(u.w)
    ci.conv_wgrad(g, y, al, be, x, u.shp, u.w.grad, xs, xt, act[0], act[1], accumulate=True, gs=gs)
    grad_ready(u.w)


def bwd_pair_into(u: Unit, g, y, al, be, x, xs, xt, epi, act, part=None, gs=None, coef=None, ent=None):
    """Data gradient + wgrad_into of a PURE expanding unit in one launch (ci.conv_bwd_pair);
    ``ent``: the layer's "bwdpair" table entry (its "wgs": the workgroups to use)."""
    if u.w.grad is None:
        u.w.grad = torch.zeros_like(u.w)
    dx, _ = ci.conv_bwd_pair(g, y, al, be, u.wd, x, u.shp, u.w.grad, epi=epi, xs=xs, xt=xt, es=xs, et=xt, act=act,
                             part=part, gs=gs, accumulate=True, coef=coef, wgs=(ent or {}).get("wgs"))
    grad_ready(u.w)
    return dx


def _rows(t):
    return t.numel() // t.shape[-1]


# CELU joins (BasicBlock, reference resnet.py:188-190): the backward takes act'(z) = exp(z/alpha)
# from the fp32 pre-activation z = y*s + t + shortcut, recomputed from the stored bf16 branch
# outputs exactly as the forward join formed it.  FDT_CELU_ZGRAD=0 restores the old derivative
# 1 + o/alpha from the bf16 join OUTPUT o, which is wrong below z ~ -0.3 (bf16 ulp of o / alpha ~
# 6.5e-3 against a derivative < 0.02) and sign-flipped for deeply negative z (o rounds below
# -alpha): the ResNet-18 convergence gap of round 5 (profiles/r6/convergence_ablation.txt).
CELU_ZGRAD = os.environ.get("FDT_CELU_ZGRAD", "1") == "1"


def _celu_jz(b, ys, sc, x_in):
    """[sa, ta, sb, tb, xid] of a CELU join's z-mode backward (None: ReLU join / disabled)."""
    if b.join[0] != ACT_CELU or not CELU_ZGRAD:
        return None
    return [ys[-1][1], ys[-1][2], sc[1] if sc else None, sc[2] if sc else None, None if sc else x_in]


# ------------------------------------------------------------------ autograd node
class ResNetBodyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_nhwc, plan: Plan, training: bool, need_grad: bool):
        nat = _native.native()
        dev = x_nhwc.device
        fs = plan.fsdp
        if fs is None:
            plan.pack(dev, need_dgrad=need_grad)
        else:
            fs.pre_forward("conv1")
            plan.pack_stage("conv1", dev, fwd=True)
        recs = []
        # stem: conv -> FCBN stats -> materialised CELU output
        st = plan.stem
        y0, (s0, t0, sm0, sa0), M0 = conv_bn_fwd(x_nhwc, st, None, None, None, training, dev)
        h = torch.empty_like(y0)
        nat.act_affine_fwd(y0.data_ptr(), s0.data_ptr(), t0.data_ptr(), h.data_ptr(), M0, st.shp.cout,
                           st.act_out[0], float(st.act_out[1]), 1, 1, _sp())
        stem_rec = (x_nhwc, y0, s0, t0, sm0, sa0)
        cur = "conv1"
        pending = None  # previous block's join, run inside this block's first conv
        pend_tile = None  # ... at this tile (_join_fold_tile)
        for bi, b in enumerate(plan.blocks):
            if fs is not None and plan.stage_of[bi] != cur:
                plan.release_stage(cur, fwd=True)
                fs.post_forward(cur)
                cur = plan.stage_of[bi]
                fs.pre_forward(cur)
                plan.pack_stage(cur, dev, fwd=True)
            x_in = h
            ys = []
            raw, s, t, act = x_in, None, None, (ACT_NONE, 1.0)
            for ui, u in enumerate(b.units):
                a_in = None
                if ui == 0 and pending is not None:
                    # writes x_in (= the previous block's output) while staging it
                    y, (su, tu, smu, sau), M = conv_bn_fwd_join(pending, u, training, dev, pend_tile)
                    pending = None
                elif MATERIALIZE_3X3 and u.shp.k > 1 and s is not None:
                    # 3x3: normalise + activate the input ONCE instead of in every one of the
                    # 9 im2col re-reads of the conv's operand staging
                    a_in = torch.empty_like(raw)
                    nat.act_affine_fwd(raw.data_ptr(), s.data_ptr(), t.data_ptr(), a_in.data_ptr(), _rows(raw),
                                       raw.shape[-1], act[0], float(act[1]), 1, 1, _sp())
                    y, (su, tu, smu, sau), M = conv_bn_fwd(a_in, u, None, None, None, training, dev)
                else:
                    y, (su, tu, smu, sau), M = conv_bn_fwd(raw, u, s, t, act, training, dev)
                ys.append((y, su, tu, smu, sau, M, a_in))
                raw, s, t, act = y, su, tu, u.act_out
            y3, s3, t3 = ys[-1][0], ys[-1][1], ys[-1][2]
            sc = None
            if b.shortcut is not None:
                u = b.shortcut
                ysc, (ssc, tsc, smsc, sasc), M = conv_bn_fwd(x_in, u, None, None, None, training, dev)
                sc = (ysc, ssc, tsc, smsc, sasc, M, None)
            out = torch.empty_like(y3)
            C = y3.shape[-1]
            # ReLU joins also emit a 1-bit-per-element activation mask: the backward reads it
            # instead of `out` (1/16 of the bytes)
            mask = None
            if need_grad and b.join[0] == ACT_RELU:
                mask = torch.empty(out.numel() // 8, device=dev, dtype=torch.uint8)
            nxt = plan.blocks[bi + 1] if bi + 1 < len(plan.blocks) else None
            pend_tile = _join_fold_tile(nxt, y3.shape) if nxt is not None and b.join[0] == ACT_RELU else None
            if pend_tile is not None:
                # the next block's first 1x1 conv computes this join while staging its operand
                # and stores `out` + mask (one pass instead of join pass + operand re-read)
                pending = (y3, s3, t3, sc[0] if sc else x_in, sc[1] if sc else None, sc[2] if sc else None, out, mask)
            else:
                nat.residual_act_fwd(y3.data_ptr(), s3.data_ptr(), t3.data_ptr(), _p(sc[0] if sc else None),
                                     _p(sc[1] if sc else None), _p(sc[2] if sc else None),
                                     0 if sc else x_in.data_ptr(), out.data_ptr(), _p(mask), _rows(y3), C, b.join[0],
                                     float(b.join[1]), 1, _sp())
            if need_grad:
                recs.append((x_in, ys, sc, out, mask))
            h = out
        if fs is not None:
            plan.release_stage(cur, fwd=True)
            fs.post_forward(cur)
        head_rec = None
        if getattr(plan, "head_on", False):
            h, head_rec = head_forward(plan.fc, h)
        if need_grad:
            ctx.plan, ctx.training = plan, training
            ctx.recs, ctx.stem_rec = recs, stem_rec
            ctx.head_rec = head_rec
        return h

    @staticmethod
    def backward(ctx, g_out):
        """Blocks in reverse order.  The gradient of a block's output arrives ALREADY through
        that block's join backward (g_pre = g*act'(out), plus its 3 statistics rows in the
        slot workspace): the next block's last dgrad -- the one that completes the gradient
        of its input -- ran the join backward in its epilogue (EPI_JOINBWD).  Only the last
        block (its gradient comes from the pooling) runs the standalone join kernel.
        Within a block the shortcut dgrad goes first (a full-coverage store of the input
        gradient; a strided shortcut writes its zero parity classes too) so the final writer
        is always the stride-1 first unit."""
        nat = _native.native()
        plan, training = ctx.plan, ctx.training
        ghw = 0  # > 0: g is the head's pooled gradient, broadcast over ghw rows per sample
        if getattr(ctx, "head_rec", None) is not None:
            g, ghw = head_backward(plan.fc, g_out, ctx.head_rec)
        else:
            g = g_out.contiguous()
        dev = g.device
        recs = ctx.recs
        nblk = len(plan.blocks)
        fs = plan.fsdp
        joined = False  # g is already g_pre of the current block (its BN-backward coefficients
        joined_coef = None  # computed with the dgrad that completed it: joined_coef)
        cur = None
        for bi in range(nblk - 1, -1, -1):
            b = plan.blocks[bi]
            if fs is not None and plan.stage_of[bi] != cur:
                if cur is not None:
                    plan.release_stage(cur, fwd=False)
                    fs.post_backward(cur)
                cur = plan.stage_of[bi]
                fs.pre_backward(cur)
                plan.pack_stage(cur, dev, fwd=False)
            x_in, ys, sc, out, mask = recs[bi]
            y3, s3 = ys[-1][0], ys[-1][1]
            C = y3.shape[-1]
            M = _rows(y3)
            part = slots(3, C, dev, M)
            if joined:
                gpre = g
            else:
                # ONE gradient g_pre = g*act'(z) for both branches: each consumer folds in its
                # own BN scale (gs = s3 / s_shortcut) in its prologue
                gpre = torch.empty_like(y3)
                jz = _celu_jz(b, ys, sc, x_in)
                nat.residual_act_bwd(g.data_ptr(), 0 if (mask is not None or jz) else out.data_ptr(), _p(mask),
                                     y3.data_ptr(), _p(sc[0] if sc else None), gpre.data_ptr(), part.data_ptr(),
                                     part.shape[0], M, C,
                                     b.join[0], float(b.join[1]), 1, _sp(), ghw, [_p(v) for v in jz] if jz else [])
                ghw = 0
            ul = b.units[-1]
            if joined:
                (al, be), coef_sc = joined_coef  # finalised with the completing dgrad (below)
            else:
                (al, be), coef_sc = bwd_finalize(part, 3, ul, (ys[-1][3], ys[-1][4], ys[-1][5]),
                                                 b.shortcut, (sc[3], sc[4], sc[5]) if sc else None, training, dev)
            assert sc is not None or len(b.units) > 1, "identity block needs >1 unit (g_pre aliasing)"
            if sc is not None:
                u = b.shortcut
                als, bes = coef_sc
                if (tuple(x_in.shape[:3]) == tuple(gpre.shape[:3]) and x_in.is_contiguous()
                        and (bpe := ci.bwd_pair_entry(x_in.shape[0], x_in.shape[1], u.shp, ci.EPI_STORE, ACT_NONE,
                                                      als is not None, False))):
                    g_x = bwd_pair_into(u, gpre, sc[0], als, bes, x_in, None, None, ci.EPI_STORE, ACT_NONE, gs=sc[1],
                                        ent=bpe)
                else:
                    g_x, _ = ci.conv_dgrad(gpre, sc[0], als, bes, u.wd, u.shp, tuple(x_in.shape), epi=ci.EPI_STORE,
                                           gs=sc[1])
                    wgrad_into(u, gpre, sc[0], als, bes, x_in, None, None, (ACT_NONE, 1.0), gs=sc[1])
            else:
                g_x = gpre  # identity: the x_in gradient accumulates onto g_pre in place
            # the block whose output is x_in: its join backward runs in the epilogue of the
            # dgrad that completes g_x (unit 0's, below) when that dgrad is dense (a strided
            # unit 0 -- BasicBlock downsampling -- writes parity classes: standalone join)
            prev = plan.blocks[bi - 1] if (bi > 0 and b.units[0].shp.stride == 1) else None
            prec = recs[bi - 1] if bi > 0 else None
            g_cur, gs_cur = gpre, s3
            # residual chain, last unit first; (al, be) = BN-backward correction of unit i
            for i in range(len(b.units) - 1, -1, -1):
                u = b.units[i]
                y, su, tu, smu, sau, Mu, a_in = ys[i]
                if i > 0:
                    yp, sp_, tp = ys[i - 1][0], ys[i - 1][1], ys[i - 1][2]
                    actp = b.units[i - 1].act_out
                    pp = slots(2, u.shp.cin, dev, _rows(yp))
                    up = b.units[i - 1]
                    cf, (al_p, be_p), _ = coef_args(up, (ys[i - 1][3], ys[i - 1][4], ys[i - 1][5]),
                                                    training=training, dev=dev)
                    if MATERIALIZE_3X3 and u.shp.k > 1:
                        # fold the BN-backward correction into the gradient once (3x3: the
                        # dgrad operand is re-read 9x, the wgrad operand once per column block)
                        gf = torch.empty_like(g_cur)
                        nat.affine_fold(g_cur.data_ptr(), y.data_ptr(), al.data_ptr(), be.data_ptr(), _p(gs_cur),
                                        gf.data_ptr(), _rows(gf), gf.shape[-1], 1, _sp())
                        g_prev, _ = ci.conv_dgrad(gf, None, None, None, u.wd, u.shp, tuple(yp.shape),
                                                  epi=ci.EPI_ACTBWD, ex=yp, es=sp_, et=tp, act=actp[0],
                                                  alpha=actp[1], part=pp, coef=cf)
                        wgrad_into(u, gf, None, None, None, a_in if a_in is not None else yp,
                                   None if a_in is not None else sp_, None if a_in is not None else tp,
                                   (ACT_NONE, 1.0) if a_in is not None else actp)
                    elif (tuple(yp.shape[:3]) == tuple(g_cur.shape[:3])
                          and (bpe := ci.bwd_pair_entry(yp.shape[0], yp.shape[1], u.shp, ci.EPI_ACTBWD, actp[0],
                                                        al is not None, True))):
                        g_prev = bwd_pair_into(u, g_cur, y, al, be, yp, sp_, tp, ci.EPI_ACTBWD, actp[0], part=pp,
                                               gs=gs_cur, coef=cf, ent=bpe)
                    else:
                        g_prev, _ = ci.conv_dgrad(g_cur, y, al, be, u.wd, u.shp, tuple(yp.shape),
                                                  epi=ci.EPI_ACTBWD, ex=yp, es=sp_, et=tp, act=actp[0],
                                                  alpha=actp[1], part=pp, gs=gs_cur, coef=cf)
                        wgrad_into(u, g_cur, y, al, be, yp, sp_, tp, actp, gs=gs_cur)
                    coef_ready(up)
                    al, be = al_p, be_p
                    g_cur, gs_cur = g_prev, None
                else:
                    if prev is not None:
                        px_in, pys, psc, pout, pmask = prec
                        pjz = _celu_jz(prev, pys, psc, px_in)
                        pul = prev.units[-1]
                        cf, ra, rb = coef_args(pul, (pys[-1][3], pys[-1][4], pys[-1][5]), prev.shortcut,
                                               (psc[3], psc[4], psc[5]) if psc else None, training, dev)
                        ci.conv_dgrad(g_cur, y, al, be, u.wd, u.shp, tuple(x_in.shape), epi=ci.EPI_JOINBWD, out=g_x,
                                      gs=gs_cur, ex=pys[-1][0], part=slots(3, x_in.shape[-1], dev, _rows(x_in)),
                                      act=prev.join[0], alpha=prev.join[1], jmask=pmask,
                                      jyb=psc[0] if psc else None,
                                      jout=None if (pmask is not None or pjz) else pout, coef=cf,
                                      es=pjz[0] if pjz else None, et=pjz[1] if pjz else None,
                                      jz=pjz[2:] if pjz else None)
                        coef_ready(pul, prev.shortcut)
                        joined_coef = (ra, rb)
                    else:
                        ci.conv_dgrad(g_cur, y, al, be, u.wd, u.shp, tuple(x_in.shape), epi=ci.EPI_ADD, out=g_x,
                                      gs=gs_cur)
                    wgrad_into(u, g_cur, y, al, be, x_in, None, None, (ACT_NONE, 1.0), gs=gs_cur)
            g = g_x
            joined = prev is not None
        if fs is not None and cur is not None:
            plan.release_stage(cur, fwd=False)
            fs.post_backward(cur)
            fs.pre_backward("conv1")
        # stem: act backward + statistics -> wgrad on the input image
        x_img, y0, s0, t0, sm0, sa0 = ctx.stem_rec
        st = plan.stem
        M0 = _rows(y0)
        C0 = st.shp.cout
        part = slots(2, C0, dev, M0)
        gy0 = torch.empty_like(y0)
        nat.act_bwd_reduce(g.data_ptr(), y0.data_ptr(), s0.data_ptr(), t0.data_ptr(), gy0.data_ptr(),
                           part.data_ptr(), part.shape[0], M0, C0, st.act_out[0], float(st.act_out[1]), 1, _sp())
        (al, be), _ = bwd_finalize(part, 2, st, (sm0, sa0, M0), training=training, dev=dev)
        wgrad_into(st, gy0, y0, al, be, x_img, None, None, (ACT_NONE, 1.0))
        if fs is not None:
            fs.post_backward("conv1")
        if not getattr(ctx, "keep", False):
            ctx.recs = ctx.stem_rec = ctx.head_rec = None
        return None, None, None, None


# ------------------------------------------------------------------ classifier head
def head_fusable(model, x, need_grad) -> bool:
    """The fused head reproduces ``fc(mean_hw(body))`` under bf16 autocast for heads of at
    most 256 classes with fp32 parameters / gradients (csrc/kernels/head.hip: up to 32 classes
    any width that is a multiple of 8; above, the MFMA head, whose tiles need a multiple of 32
    channels); anything else keeps the PyTorch ops."""
    fc = getattr(model, "fc", None)
    if not FUSED_HEAD or not getattr(model, "fused_head", True) or not isinstance(fc, nn.Linear) or fc.bias is None or getattr(model, "_fsdp", None) is not None:
        return False
    if not isinstance(getattr(model, "avg_pool", None), nn.AdaptiveAvgPool2d) or fc._forward_hooks or fc._forward_pre_hooks:
        return False
    dt = x.device.type
    if not (torch.is_autocast_enabled(dt) and torch.get_autocast_dtype(dt) == BF16):
        return False
    if not hasattr(_native.native(), "head_fwd"):
        return False
    K, C = fc.weight.shape
    if K > HEAD_MAX_CLASSES or C % (32 if K > 32 else 8):
        return False
    for p in (fc.weight, fc.bias):
        if p.dtype != torch.float32 or not p.is_contiguous() or (need_grad and not p.requires_grad):
            return False
        if p.grad is not None and (p.grad.dtype != torch.float32 or not p.grad.is_contiguous()):
            return False
    return True


def head_forward(fc, h):
    """body [N,H,W,C] bf16 -> (logits [N,K] bf16, (pooled bf16 [N,C], H*W))."""
    N, H, W, C = h.shape
    K = fc.weight.shape[0]
    pooled = torch.empty(N, C, device=h.device, dtype=BF16)
    logits = torch.empty(N, K, device=h.device, dtype=BF16)
    _native.native().head_fwd(h.data_ptr(), fc.weight.data_ptr(), fc.bias.data_ptr(), pooled.data_ptr(),
                              logits.data_ptr(), N, H * W, C, K, _sp())
    return logits, (pooled, H * W)


def head_backward(fc, g_logits, rec):
    """Accumulates fc.weight.grad / fc.bias.grad (signalling their readiness) and returns
    the pooled gradient [N,C] bf16 (already / HW) with its broadcast row count HW."""
    pooled, hw = rec
    N, C = pooled.shape
    K = fc.weight.shape[0]
    dl = g_logits.to(BF16).contiguous()
    for p in (fc.weight, fc.bias):
        if p.grad is None:
            p.grad = torch.zeros_like(p)
    dpool = torch.empty(N, C, device=pooled.device, dtype=BF16)
    _native.native().head_bwd(dl.data_ptr(), fc.weight.data_ptr(), pooled.data_ptr(), dpool.data_ptr(),
                              fc.weight.grad.data_ptr(), fc.bias.grad.data_ptr(), N, hw, C, K, _sp())
    grad_ready(fc.bias)
    grad_ready(fc.weight)
    return dpool, hw


def to_engine_input(x: torch.Tensor, cxp: int = 8) -> torch.Tensor:
    """(N,3,H,W) image batch (any layout/dtype) -> (N,H,W,cxp) bf16 zero-padded NHWC.
    Zero-copy when x is the channel-sliced NCHW view of such a buffer (the device CIFAR
    loader produces exactly that)."""
    N, C, H, W = x.shape
    if x.dtype == BF16 and x.stride() == (H * W * cxp, 1, W * cxp, cxp):
        return torch.as_strided(x, (N, H, W, cxp), (H * W * cxp, W * cxp, cxp, 1))
    out = torch.zeros(N, H, W, cxp, device=x.device, dtype=BF16)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return out


def resnet_engine_forward(model, x):
    """Forward of ``models.resnet.ResNet`` through the engine; returns logits."""
    plan = getattr(model, "_plan", None)
    if plan is None:
        plan = model._plan = Plan(model)
    plan.fsdp = getattr(model, "_fsdp", None)
    # FSDP: graph segments between the stages only in static mode (persistent buffers; the
    # collectives run as actions between segments); eager otherwise
    plan.use_graphs = bool(getattr(model, "graph_engine", False)) and (plan.fsdp is None or plan.fsdp.static)
    xin = to_engine_input(x, plan.stem.shp.cxp)
    need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in model.parameters())
    if not model.training and getattr(model, "eval_stats", "batch") == "running":
        return resnet_frozen_forward(model, x)  # (refuses gradients and FSDP models itself)
    plan.fc = model.fc
    plan.head_on = head_fusable(model, x, need_grad)
    if need_grad:
        # the engine writes weight gradients itself; autograd sees one node whose only
        # differentiable input is a dummy (the image batch needs no gradient)
        dummy = torch.empty(0, device=x.device, requires_grad=True)
        body = _BodyWithDummy.apply(xin, dummy, plan, model.training)
    else:
        body = ResNetBodyFn.forward(_NoCtx(), xin, plan, model.training, False)
    if plan.head_on:
        return body  # logits of the fused head
    pooled = body.mean(dim=(1, 2), dtype=torch.float32)  # fp32 accumulation, no fp32 copy of the body
    return model.fc(pooled)


# ------------------------------------------------------------------ frozen inference
# Eval forward with FROZEN statistics (model.eval_stats == "running"): every unit's scale and
# shift are known before its conv runs, so normalisation, activation and the residual join move
# into the conv's epilogue (conv_igemm_impl.h EPI_NORMACT) -- one launch per convolution, plus the
# weight pack, the coefficient kernel (bn_frozen_coef: every unit's (s, t) from the current
# running statistics, at fixed addresses) and the head.  No statistics, finalize, normalise, join
# or mask launches; no reduction crosses the rows of the batch.
FROZEN_GRAPH_SHAPES = 4  # captured input shapes kept per model (oldest dropped first)


class _FrozenCoef:
    """(s, t) of every unit in one flat fp32 buffer + the table bn_frozen_coef fills it from."""

    def __init__(self, plan, dev):
        rows, off, self.views = [], 0, {}
        for u in plan.units:
            C = u.shp.cout
            if u.bn is None:
                if not u.fc.track_running_stats:
                    raise RuntimeError("frozen forward: FusedConvBN without running statistics (enable_running_stats)")
                src = (u.fc.running_mean, u.fc.running_var, None, None)
            else:
                if not u.bn.track_running_stats:
                    raise RuntimeError("frozen forward: BatchNorm2d without running statistics")
                src = (u.bn.running_mean, u.bn.running_var, u.bn.weight, u.bn.bias)
            for t in src:
                assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and t.numel() == C and t.device == dev)
            eps_bits = struct.unpack("<q", struct.pack("<d", float(u.eps)))[0]
            rows.append([_p(src[0]), _p(src[1]), _p(src[2]), _p(src[3]), C, off, 0 if u.bn is None else 1, eps_bits])
            self.views[id(u)] = (off, C)
            off += 2 * C
        self.key = _FrozenCoef.key_of(plan, dev)
        self.table = torch.tensor(rows, dtype=torch.int64, device=dev)
        self.buf = torch.empty(off, device=dev, dtype=torch.float32)
        self.n = len(rows)

    @staticmethod
    def key_of(plan, dev):
        ptrs = []
        for u in plan.units:
            m = u.fc if u.bn is None else u.bn
            ptrs += [_p(getattr(m, "running_mean", None)), _p(getattr(m, "running_var", None))]
            if u.bn is not None:
                ptrs += [_p(u.bn.weight), _p(u.bn.bias)]
            ptrs.append(_p(u.w))  # (a captured forward packs from, and so bakes in, the weights' storage)
        fc = getattr(plan, "fc", None)
        if fc is not None:
            ptrs += [_p(fc.weight), _p(fc.bias)]
        return (str(dev), tuple(ptrs))

    def fill(self):
        _native.native().bn_frozen_coef(self.table.data_ptr(), self.n, self.buf.data_ptr(), _sp())

    def st(self, u):
        off, C = self.views[id(u)]
        return self.buf[off:off + C], self.buf[off + C:off + 2 * C]


def _frozen_body(plan, xin, coef):
    """Stem + blocks (+ the fused head) on ``xin`` (engine input layout), frozen statistics."""
    dev = xin.device
    plan.pack(dev, need_dgrad=False)
    coef.fill()

    # deterministic mode: K is never split over workgroups, so every convolution sums K in one
    # order whatever the batch size -- split-K factors follow the row count, and a batch of one
    # (split 4-8) otherwise differs from the same image inside a batch of 64 (split 1-4) by single
    # bf16 roundings that a deep network amplifies (2.4e-2 of the logits of a random-init,
    # freshly calibrated ResNet-50: profiles/x2/README.md)
    ns = 1 if _native.deterministic() else None

    def conv(x, u, act, res=None):
        return ci.conv_fwd(x, u.wf, u.shp, norm=coef.st(u), res=res, out_act=act, nsplit=ns)[0]

    h = conv(xin, plan.stem, plan.stem.act_out)
    for b in plan.blocks:
        x_in = h
        # the shortcut conv stores its normalised output: the residual of the block's last unit
        r = conv(x_in, b.shortcut, (ACT_NONE, 1.0)) if b.shortcut is not None else x_in
        for i, u in enumerate(b.units):
            last = i + 1 == len(b.units)
            h = conv(h, u, b.join if last else u.act_out, r if last else None)
    if getattr(plan, "head_on", False):
        h, _ = head_forward(plan.fc, h)
    return h


class _FrozenGraph:
    def __init__(self):
        self.stage = "warm"   # warm (ran eagerly once) -> ready (captured; calls replay)
        self.pool = self.x = self.h = self.rec = None
        self.replays = 0


def _frozen_coef(plan, dev):
    coef = plan.__dict__.get("_frozen_coef")
    if coef is None or coef.key != _FrozenCoef.key_of(plan, dev):
        coef = plan._frozen_coef = _FrozenCoef(plan, dev)
        # captured against the old buffers (statistics, affine) or parameters re-pointed since
        # (model.to, a flat parameter space built later, param.data = ...)
        plan.__dict__.pop("_frozen_graphs", None)
    return coef


def resnet_frozen_forward(model, x):
    """Eval forward of ``models.resnet.ResNet`` with frozen (running) statistics; returns logits.
    With ``model.graph_engine`` the forward of each input shape is captured once (static input /
    output, a private pool per capture) on its second call and replayed afterwards."""
    if getattr(model, "_fsdp", None) is not None:
        raise RuntimeError("eval_stats='running' is not supported on an FSDP-sharded model")
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in model.parameters())):
        raise RuntimeError("the frozen forward keeps nothing for a backward: run it under torch.no_grad()")
    plan = getattr(model, "_plan", None)
    if plan is None:
        plan = model._plan = Plan(model)
    plan.fsdp = None
    xin = to_engine_input(x, plan.stem.shp.cxp)
    dev = xin.device
    plan.fc = model.fc
    plan.head_on = head_fusable(model, x, False)
    coef = _frozen_coef(plan, dev)
    st = None
    if bool(getattr(model, "graph_engine", False)) and os.environ.get("FDT_GRAPHS", "1") != "0":
        cache = plan.__dict__.setdefault("_frozen_graphs", OrderedDict())
        key = (tuple(xin.shape), plan.head_on, _native.deterministic())
        st = cache.get(key)
        if st is None:
            st = cache[key] = _FrozenGraph()  # this call: eager warm-up (workspaces, kernel attributes)
            while len(cache) > FROZEN_GRAPH_SHAPES:
                cache.popitem(last=False)
            st = None
        elif st.stage == "warm":
            st.pool = torch.cuda.graph_pool_handle()
            st.x = xin.clone()
            cur = torch.cuda.current_stream()
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            torch.cuda.synchronize()
            rec = _graphs.Recorder(st.pool)
            with torch.cuda.stream(side), _graphs.recording(rec), _graphs.capture_guard():
                rec.begin()
                try:
                    st.h = _frozen_body(plan, st.x, coef)
                finally:
                    rec.end()
            cur.wait_stream(side)
            st.rec = rec
            st.stage = "ready"
    if st is not None:
        st.x.copy_(xin)
        st.rec.replay()
        st.replays += 1
        body = st.h
        if plan.head_on:
            return body.clone()  # (the static output is overwritten by the next replay)
    else:
        body = _frozen_body(plan, xin, coef)
        if plan.head_on:
            return body
    pooled = body.mean(dim=(1, 2), dtype=torch.float32)
    return model.fc(pooled)


class _NoCtx:
    pass


class _GraphState:
    """HIP graphs of one (batch shape, train/eval) configuration of the body.

    Step 1 runs eagerly (warm-up: lazy kernel attributes, slot workspace, allocator).
    Step 2 captures the forward into one graph and the backward into segments cut where a
    gradient bucket becomes ready, then replays them.  Later steps copy the batch into the
    static input, replay the forward graph, and in backward copy the incoming gradient and
    replay the segments, launching each bucket's all-reduce between them.  Every kernel of
    the body (~400 at ResNet-50) is then one graph launch per segment: the host no longer
    paces the GPU at small per-GPU batches (the 8-GPU case)."""

    def __init__(self):
        self.stage = "warm"
        self.pool = None
        self.x = self.h = self.g = None
        self.inner = None
        self.fwd = None
        self.segments = None
        self.repacks = True


def graphs_enabled(plan) -> bool:
    return getattr(plan, "use_graphs", False) and os.environ.get("FDT_GRAPHS", "1") != "0"


class _BodyWithDummy(torch.autograd.Function):
    """Gives the body node a differentiable input so autograd calls its backward even
    though the image batch does not require grad.  With graphs enabled the body runs as
    captured HIP graphs (see ``_GraphState``)."""

    @staticmethod
    def forward(ctx, xin, dummy, plan, training):
        st = None
        if graphs_enabled(plan):
            # (the tracked units' momenta are scalars of the captured finalize launches, and their
            # sign decides whether the count's increment kernel is captured at all)
            key = (tuple(xin.shape), bool(training), bool(getattr(plan, "head_on", False)), plan.tracking())
            states = plan.__dict__.setdefault("_graphs", {})
            st = states.get(key)
            if st is None:
                states[key] = _GraphState()  # this step: eager warm-up
            elif st.stage == "warm":
                st.pool = torch.cuda.graph_pool_handle()
                st.x = xin.clone()
                st.inner = _NoCtx()
                st.inner.keep = True
                # forward as graph segments: one, or (static FSDP) one per stage with each
                # unit's all-gather wait / next-unit prefetch as actions between them
                cur = torch.cuda.current_stream()
                side = torch.cuda.Stream()
                side.wait_stream(cur)
                torch.cuda.synchronize()
                rec = _graphs.Recorder(st.pool)
                st.repacks = not plan.pack_fresh()  # does the captured forward repack the weights?
                with torch.cuda.stream(side), _graphs.recording(rec), _graphs.capture_guard():
                    rec.begin()
                    try:
                        st.h = ResNetBodyFn.forward(st.inner, st.x, plan, training, True)
                    finally:
                        rec.end()
                cur.wait_stream(side)
                st.fwd = rec
                st.fwd.replay()
                st.stage = "fwd"
            else:
                if not st.repacks and not plan.pack_fresh():
                    # captured without the repack (the optimizer packs): weights written since by
                    # something else -- repack before the replay
                    plan.pack(xin.device, need_dgrad=True)
                st.x.copy_(xin)
                st.fwd.replay()
        ctx.gstate = st if (st is not None and st.stage in ("fwd", "ready")) else None
        if ctx.gstate is not None:
            return st.h.detach()
        ctx.inner = _NoCtx()
        return ResNetBodyFn.forward(ctx.inner, xin, plan, training, True)

    @staticmethod
    def backward(ctx, g):
        st = ctx.gstate
        if st is None:
            ResNetBodyFn.backward(ctx.inner, g)
            return None, None, None, None
        if st.stage == "fwd":
            st.g = g.detach().clone().contiguous()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            torch.cuda.synchronize()
            rec = _graphs.Recorder(st.pool)
            with torch.cuda.stream(side), _graphs.recording(rec), _graphs.capture_guard():
                rec.begin()
                try:
                    ResNetBodyFn.backward(st.inner, st.g)
                finally:
                    rec.end()
            torch.cuda.current_stream().wait_stream(side)
            st.rec = rec
            st.segments = rec.segments
            st.stage = "ready"
        else:
            st.g.copy_(g)
        st.rec.replay()
        if st.rec.needs_check:
            # first replay of a backward whose bucket all-reduces were captured in-graph:
            # checked against eager all-reduces (parallel/graphs.py); the checking graph (it
            # snapshots every bucket) is dropped and the next step recaptures the backward --
            # in capture mode, or with cuts if the check failed
            st.rec.check_collectives()
            st.stage, st.rec, st.segments = "fwd", None, None
        return None, None, None, None

"""Packed variable-length attention (csrc/kernels/attention_varlen.hip) row by row against the
fp64 oracle of attention_oracle.py run one sequence at a time, and the packed Transformer
forward against the padded one.

Budget: row_err(kernel, oracle) <= 2 x row_err(bf16 arm, oracle) for O, dQ, dK, dV; slack rows
(past cu[B]) exactly zero.

Worst measured kernel/arm ratio on an MI355X over the cases of this file (row errors kernel /
arm, and the case):
    O    0.44   3.12e-3 / 7.08e-3   dropout p=0.5
    dQ   0.72   5.92e-3 / 8.28e-3   (97, 5, 128) H=3 slack=7
    dK   0.67   6.13e-3 / 9.12e-3   (1, 64, 65, 2) H=8 slack=7
    dV   0.65   4.04e-3 / 6.22e-3   (31, 32, 33) H=3 slack=7
At (1,) (zero dQ, dK) the largest row norm was 2.1e-6 against a limit of 7.8e-3.  The CPU model
test measured 3.4e-7 (logits) and 7.3e-7 (gradients) against its 1e-5.
"""
import copy
import functools
import math

import pytest
import torch

import attention_oracle as ao

gpu = pytest.mark.gpu
NAMES = ("O", "dQ", "dK", "dV")


def _cu(lens, device):
    return torch.tensor([0] + list(lens), dtype=torch.int32).cumsum(0).to(device, torch.int32)


def _inputs(lens, H, slack, seed, device, qscale=1.0):
    """(T, 3, H, 64) bf16 packed projection and a (T, H, 64) output gradient; slack rows hold
    ordinary random values, which the kernels must not let through."""
    T = sum(lens) + slack
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(T, 3, H, 64, generator=g)
    qkv[:, 0] *= qscale
    go = torch.randn(T, H, 64, generator=g)
    return qkv.to(device, torch.bfloat16), go.to(device, torch.bfloat16)


def _run(qkv, go, cu, max_len, p=0.0):
    from faster_distributed_training_amd.ops import attention_native as an
    x = qkv.detach().clone().requires_grad_()
    out = an.attention_varlen_packed(x, cu, max_len, p)
    out.backward(go)
    return (out.detach(),) + tuple(x.grad.unbind(1))


def _per_sequence(fn, qkv, go, lens, keep=None, p=0.0):
    """fn (ao.oracle / ao.bf16_arm) on every sequence as a batch of one -> (O, dQ, dK, dV), each
    (1, sum(lens), H, 64)."""
    outs, s0 = [], 0
    for n in lens:
        if n:
            q, k, v = qkv[s0:s0 + n].unsqueeze(0).unbind(2)
            kp = None if keep is None else keep[:, :, s0:s0 + n, s0:s0 + n]
            outs.append(fn(q, k, v, None, None, keep=kp, p=p, go=go[s0:s0 + n].unsqueeze(0)))
        s0 += n
    return tuple(torch.cat(ts, 1) for ts in zip(*outs))


def _check(tag, got, qkv, go, lens, keep=None, p=0.0):
    n = sum(lens)
    ref = _per_sequence(ao.oracle, qkv, go, lens, keep, p)
    arm = _per_sequence(ao.bf16_arm, qkv, go, lens, keep, p)
    lines, bad = [], []
    for name, g, a, r in zip(NAMES, got, arm, ref):
        assert torch.isfinite(g).all(), name
        assert (g[n:] == 0).all(), f"{name}: slack rows not zero"
        ok, text = ao.budget_report(name, g[:n].unsqueeze(0), a, r, ref[3])
        lines.append(text)
        if not ok:
            bad.append(text)
    print(f"BUDGET {tag} | " + " | ".join(lines))
    assert not bad, (tag, bad)


LENS = ((1,), (31, 32, 33), (1, 64, 65, 2), (97, 5, 128), (129, 0, 40))
CASES = [pytest.param(lens, H, slack, 0, 1.0, id=f"{'_'.join(map(str, lens))}-H{H}-s{slack}")
         for lens in LENS for H in (3, 8) for slack in (0, 7)]
CASES.append(pytest.param((97, 5, 128), 8, 7, 31, 1.0, id="97_5_128-maxlen+31"))
CASES.append(pytest.param((129, 40), 3, 7, 0, 4.0, id="129_40-q4"))  # the running maximum moves between tiles


@gpu
@pytest.mark.parametrize("lens,H,slack,extra,qscale", CASES)
def test_varlen_rows_against_oracle(cuda, lens, H, slack, extra, qscale):
    """Every (row, head) of O, dQ, dK, dV within the budget of the per-sequence fp64 oracle, at
    lengths around the 32-row tile, with an idle wave (H = 3), an empty sequence and slack."""
    qkv, go = _inputs(lens, H, slack, sum(lens) + H, cuda, qscale)
    got = _run(qkv, go, _cu(lens, cuda), max(lens) + extra)
    _check(f"varlen {lens} H={H} slack={slack} max_len+{extra} q*{qscale:g}", got, qkv, go, lens)


@gpu
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_varlen_dropout(cuda, p):
    """The keep mask read out of the forward (V = unit vectors) never crosses a sequence, has the
    binomial share of kept entries, and is the mask both backward kernels use."""
    from faster_distributed_training_amd.ops import attention_native as an
    lens, H, seed = (70, 33), 2, 4321
    T = sum(lens)
    qkv, go = _inputs(lens, H, 0, 11, cuda)
    cu = _cu(lens, cuda)

    def fwd(q, k, v):
        return an.attention_varlen_packed(torch.stack([q[0], k[0], v[0]], 1), cu, max(lens), p).unsqueeze(0)

    q, k = qkv[:, 0].unsqueeze(0), qkv[:, 1].unsqueeze(0)
    Pd = ao.recover_pdrop(fwd, q, k, T, seed)                      # (1, H, T, T)
    seq = torch.repeat_interleave(torch.arange(len(lens)), torch.tensor(lens)).to(cuda)
    live = (seq[:, None] == seq[None, :]).expand(1, H, T, T)
    assert (Pd[~live] == 0).all(), "probability between two sequences"
    S = torch.einsum("qhd,khd->hqk", qkv[:, 0].double(), qkv[:, 1].double()) / 8.0
    P = torch.softmax(S.masked_fill(~live[0], float("-inf")), -1)[None]
    assert (P[live] > 1e-30).all(), "ambiguous entries: a zero could be a dropped or a vanished probability"
    keep = (Pd != 0) | ~live
    n = int(live.sum())
    share, sigma = keep[live].double().mean().item(), math.sqrt(p * (1 - p) / n)
    print(f"DROPOUT p={p}: kept {share:.5f} of {n}, expected {1 - p} +- 4 x {sigma:.5f}")
    assert abs(share - (1 - p)) <= 4 * sigma
    torch.manual_seed(seed)
    _check(f"varlen dropout p={p}", _run(qkv, go, cu, max(lens), p), qkv, go, lens, keep, p)


@gpu
def test_varlen_bitwise_repeatable(cuda):
    """No atomics: the same seed gives the same bits, also with cu_seqlens at another address."""
    lens, H = (97, 5, 128), 3
    qkv, go = _inputs(lens, H, 7, 3, cuda)
    cu = _cu(lens, cuda)
    moved = torch.cat([cu.new_zeros(61), cu])[61:]
    assert moved.data_ptr() != cu.data_ptr()
    runs = []
    for c in (cu, cu, moved):
        torch.manual_seed(99)
        runs.append(_run(qkv, go, c, max(lens), 0.1))
    for other in runs[1:]:
        for name, a, b in zip(NAMES, runs[0], other):
            assert torch.equal(a, b), name


# ------------------------------------------------------------------------------ model
LENGTHS = (5, 33, 1, 17)


@functools.lru_cache(maxsize=None)
def _model_and_batch():
    from faster_distributed_training_amd.models.transformer import Transformer
    torch.manual_seed(0)
    model = Transformer(4, 100, n_layers=2, h=8, d_model=512, d_ff=1024, d_hidden=1024, maxlen=64).eval()
    L = max(LENGTHS)
    ids = torch.randint(1, 100, (len(LENGTHS), L))
    types = torch.randint(0, 2, (len(LENGTHS), L))
    return model, ids, types


def _model_run(device, packed, autocast=False):
    """(logits, {name: grad}) of logits.sum() on a copy of the shared model, as fp64 on the CPU."""
    from faster_distributed_training_amd.models.transformer import pack_tokens
    model, ids, types = _model_and_batch()
    model = copy.deepcopy(model).to(device)
    ids, types = ids.to(device), types.to(device)
    L = ids.size(1)
    index = torch.arange(64, device=device)
    with torch.autocast(device.type, dtype=torch.bfloat16, enabled=autocast):
        if packed:
            pids, ptypes, cu, max_len = pack_tokens(ids, types, LENGTHS, multiple=16)
            assert pids.shape == (1, 64) and cu.tolist() == [0, 5, 38, 39, 56] and max_len == 33
            logits, _, _ = model(pids, ptypes, index, cu_seqlens=cu, max_len=max_len)
        else:
            mask = (torch.arange(L)[None, :] < torch.tensor(LENGTHS)[:, None]).long().to(device)
            logits, _, _ = model(ids, types, index, mask.view(len(LENGTHS), 1, 1, L))
    logits.float().sum().backward()
    return logits.detach().double().cpu(), {n: p.grad.detach().double().cpu() for n, p in model.named_parameters()}


@functools.lru_cache(maxsize=None)
def _cpu_padded():
    return _model_run(torch.device("cpu"), packed=False)


def _model_err(run, ref):
    """(logit error, worst parameter-gradient error), each relative to the reference's norm; a
    gradient's norm is floored by 1e-3 of the largest one (the key bias has a zero gradient)."""
    floor = 1e-3 * max(g.norm().item() for g in ref[1].values())
    e_logit = ((run[0] - ref[0]).norm() / ref[0].norm()).item()
    e_grad = max(((run[1][n] - g).norm() / (g.norm() + floor)).item() for n, g in ref[1].items())
    return e_logit, e_grad


def test_packed_model_matches_padded_cpu():
    """fp32 on the CPU: the packed forward and backward are the padded ones up to reassociation."""
    from faster_distributed_training_amd.models.transformer import Transformer
    e_logit, e_grad = _model_err(_model_run(torch.device("cpu"), packed=True), _cpu_padded())
    print(f"MODEL cpu packed vs padded: logits {e_logit:.3e} gradients {e_grad:.3e}")
    assert e_logit <= 1e-5 and e_grad <= 1e-5
    with pytest.raises(ValueError):
        Transformer(4, 100, n_layers=1, maxlen=64, faithful=True)(
            torch.zeros(1, 8, dtype=torch.long), torch.zeros(1, 8, dtype=torch.long), None,
            cu_seqlens=torch.tensor([0, 8], dtype=torch.int32), max_len=8)


@gpu
def test_packed_model_on_kernels(cuda):
    """bf16 autocast on the kernels: the packed run is as close to the fp32 CPU model as the
    padded run is, within the budget factor.  Measured on an MI355X: padded logits 5.2e-3,
    gradients 4.9e-2; packed logits 5.6e-3, gradients 6.1e-2."""
    pad = _model_err(_model_run(cuda, packed=False, autocast=True), _cpu_padded())
    pack = _model_err(_model_run(cuda, packed=True, autocast=True), _cpu_padded())
    print(f"MODEL gpu vs fp32 cpu: padded logits {pad[0]:.3e} grads {pad[1]:.3e} | "
          f"packed logits {pack[0]:.3e} grads {pack[1]:.3e}")
    assert pack[0] <= ao.BUDGET * pad[0] and pack[1] <= ao.BUDGET * pad[1]

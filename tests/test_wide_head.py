"""The wide classifier head (csrc/kernels/head.hip, 32 < classes <= 256): the kernels against
the fp32 PyTorch head, their tails, row independence and repeatability, and the engine running
a 100-class head inside its graphs (training step and frozen forward)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
GUARD = 64


def rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def guarded(shape, dtype, device, init=None):
    """A contiguous tensor of ``shape`` (NaN, or a copy of ``init``) followed in the same
    allocation by GUARD elements of 7.0; returns (tensor, guard view)."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + GUARD,), 7.0, device=device, dtype=dtype)
    t = buf[:n].view(*shape)
    if init is None:
        t.fill_(float("nan"))
    else:
        t.copy_(init)
    return t, buf[n:]


def guard_intact(g):
    return bool((g == 7.0).all())


def head_inputs(cuda, N, K, C, HW):
    g = torch.Generator(device=cuda).manual_seed(N + K)
    body = torch.randn(N, HW, C, device=cuda, generator=g).relu().to(BF)
    W = torch.randn(K, C, device=cuda, generator=g) * C ** -0.5
    b = torch.randn(K, device=cuda, generator=g)
    return g, body, W, b


def run_fwd(nat, body, W, b):
    N, HW, C = body.shape
    K = W.shape[0]
    pooled, gp = guarded((N, C), BF, body.device)
    logits, gl = guarded((N, K), BF, body.device)
    nat.head_fwd(body.data_ptr(), W.data_ptr(), b.data_ptr(), pooled.data_ptr(), logits.data_ptr(), N, HW, C, K,
                 _stream())
    torch.cuda.synchronize()
    assert guard_intact(gp) and guard_intact(gl)
    return pooled, logits


def run_bwd(nat, dl, W, pooled, gW0, gb0, HW):
    N, K = dl.shape
    C = W.shape[1]
    gW, ggW = guarded((K, C), torch.float32, dl.device, gW0)
    gb, ggb = guarded((K,), torch.float32, dl.device, gb0)
    dpool, gdp = guarded((N, C), BF, dl.device)
    nat.head_bwd(dl.data_ptr(), W.data_ptr(), pooled.data_ptr(), dpool.data_ptr(), gW.data_ptr(), gb.data_ptr(),
                 N, HW, C, K, _stream())
    torch.cuda.synchronize()
    assert guard_intact(ggW) and guard_intact(ggb) and guard_intact(gdp)
    return dpool, gW, gb


@pytest.mark.parametrize("N,K,C,HW", [(1, 100, 512, 16), (33, 33, 64, 1), (96, 100, 2048, 16), (257, 200, 512, 49),
                                      (128, 256, 2048, 16)])
def test_wide_head_kernels_match_fp32(cuda, N, K, C, HW):
    """head_fwd / head_bwd above 32 classes against the fp32 PyTorch head fc(mean_hw(body)) and
    its gradients: the tolerances of test_fused_head_kernels_match_fp32.  Outputs start as NaN
    (an unwritten tail element fails the comparison) and the 64 elements after each output stay
    untouched."""
    from faster_distributed_training_amd.ops import _native
    nat = _native.native()
    g, body, W, b = head_inputs(cuda, N, K, C, HW)
    pooled, logits = run_fwd(nat, body, W, b)
    p_ref = body.float().mean(1)
    l_ref = p_ref @ W.t() + b
    print(f"pooled {rel(pooled, p_ref):.3e} logits {rel(logits, l_ref):.3e}")
    assert rel(pooled, p_ref) < 4e-3
    assert rel(logits, l_ref) < 1e-2, rel(logits, l_ref)
    dl = torch.randn(N, K, device=cuda, generator=g).to(BF)
    gW0 = torch.randn(K, C, device=cuda, generator=g)
    gb0 = torch.randn(K, device=cuda, generator=g)
    dpool, gW, gb = run_bwd(nat, dl, W, pooled, gW0, gb0, HW)
    e_dp, e_gw = rel(dpool, dl.float() @ W / HW), rel(gW - gW0, dl.float().t() @ p_ref)
    e_gb = rel(gb - gb0, dl.float().sum(0))
    print(f"dpool {e_dp:.3e} gW {e_gw:.3e} gb {e_gb:.3e}")
    assert e_dp < 1e-2
    assert e_gw < 1e-2
    assert e_gb < 1e-4


def test_wide_head_rows_independent(cuda):
    """The logits and pooled values of a sample depend neither on the other rows nor on N: row 0
    alone and rows 0..32 give the bits they have in the batch of 64."""
    from faster_distributed_training_amd.ops import _native
    nat = _native.native()
    _, body, W, b = head_inputs(cuda, 64, 100, 2048, 16)
    p64, l64 = run_fwd(nat, body, W, b)
    for n in (1, 33):
        p, l = run_fwd(nat, body[:n].contiguous(), W, b)
        assert torch.equal(p, p64[:n]) and torch.equal(l, l64[:n]), n
    assert not torch.isnan(l64.float()).any()


def test_wide_head_backward_repeatable(cuda):
    """One owner and a fixed summation order per output element: two calls from the same inputs
    and initial gradients agree bitwise."""
    from faster_distributed_training_amd.ops import _native
    nat = _native.native()
    N, K, C, HW = 200, 100, 2048, 16
    g, body, W, b = head_inputs(cuda, N, K, C, HW)
    pooled, _ = run_fwd(nat, body, W, b)
    dl = torch.randn(N, K, device=cuda, generator=g).to(BF)
    gW0 = torch.randn(K, C, device=cuda, generator=g)
    gb0 = torch.randn(K, device=cuda, generator=g)
    a = run_bwd(nat, dl, W, pooled, gW0, gb0, HW)
    c = run_bwd(nat, dl, W, pooled, gW0, gb0, HW)
    for u, v in zip(a, c):
        assert not torch.isnan(u.float()).any() and torch.equal(u, v)


def test_engine_fuses_100_class_head(cuda):
    """ResNet-18 with 100 classes, batch 32, bf16 autocast, deterministic mode, a loss linear in
    the logits: the engine runs the head itself (``head_on``), its logits and gradients match the
    PyTorch head on the same engine within the bounds of
    test_engine_fused_head_matches_pytorch_head, the fc gradients fire the grad-ready hook once
    each, and a replayed graph step equals the eager one within the same bounds."""
    from faster_distributed_training_amd.models import resnet as R
    from faster_distributed_training_amd.ops import _native
    from faster_distributed_training_amd.ops import resnet_fused as rf
    from faster_distributed_training_amd.ops.resnet_fused import register_grad_ready_hook
    from faster_distributed_training_amd.utils.flat import FlatParams
    torch.manual_seed(0)
    m = R.resnet18(100).to(cuda)
    m.fast_path = True
    m.graph_engine = False
    flat = FlatParams(m, device=cuda)  # persistent gradients (the captured graphs write them in place)
    x = torch.randn(32, 3, 32, 32, device=cuda)
    r = torch.randn(32, 100, device=cuda).to(BF).float()

    def step():
        flat.grad.zero_()
        with torch.autocast("cuda", dtype=BF):
            out = m(x)
        (out.float() * r).sum().backward()
        torch.cuda.synchronize()
        return out.detach().float().clone(), {n: p.grad.clone() for n, p in m.named_parameters()}

    def check(of, gf, o1, g1):
        assert rel(of, o1) < 1e-2, rel(of, o1)
        errs = {n: rel(gf[n], g1[n]) for n in g1}
        print("worst gradient differences:", sorted(errs.items(), key=lambda kv: -kv[1])[:4])
        assert errs["fc.weight"] < 1e-2 and errs["fc.bias"] < 1e-2, (errs["fc.weight"], errs["fc.bias"])
        assert max(v for n, v in errs.items() if not n.startswith("fc.")) < 1e-3
        flat_f = torch.cat([gf[n].flatten() for n in g1])
        flat_1 = torch.cat([g1[n].flatten() for n in g1])
        assert rel(flat_f, flat_1) < 2e-2, rel(flat_f, flat_1)

    saved = rf.FUSED_HEAD
    _native.set_deterministic(True)
    try:
        rf.FUSED_HEAD = False
        o1, g1 = step()
        assert not m._plan.head_on
        rf.FUSED_HEAD = True
        seen = []
        hs = [register_grad_ready_hook(p, lambda q: seen.append(id(q))) for p in (m.fc.weight, m.fc.bias)]
        of, gf = step()
        assert m._plan.head_on
        assert sorted(seen) == sorted([id(m.fc.weight), id(m.fc.bias)])
        for h in hs:
            h.remove()
        check(of, gf, o1, g1)
        m.graph_engine = True
        for _ in range(3):  # warm-up, capture + replay, replay
            og, gg = step()
        (st,) = [s for k, s in m._plan._graphs.items() if k[2]]
        assert st.stage == "ready" and m._plan.head_on
        check(og, gg, of, gf)
    finally:
        rf.FUSED_HEAD = saved
        _native.set_deterministic(False)


def test_frozen_forward_100_classes_in_graph(cuda, monkeypatch):
    """Frozen (running-statistics) inference of a 100-class ResNet-18 under graph replay: logits
    within the bound of test_frozen_forward_matches_fp32_oracle of the fp32 model fed the same
    statistics; batch 1 equals row 0 of a batch of 64 bit for bit (deterministic mode); the native
    calls end in head_fwd and no torch mean / linear follows the replay."""
    import torch.nn.functional as F
    from torch.utils._python_dispatch import TorchDispatchMode
    from faster_distributed_training_amd.models import resnet as R
    from faster_distributed_training_amd.ops import _native
    torch.backends.cudnn.allow_tf32 = False
    torch.manual_seed(0)
    m_ref, m = R.resnet18(100).to(cuda), R.resnet18(100).to(cuda)
    m.load_state_dict(m_ref.state_dict())
    m_ref.fast_path, m.fast_path = False, True
    for u in (m_ref, m):
        R.enable_running_stats(u)
    g = torch.Generator().manual_seed(4)
    y = torch.randint(0, 100, (32,), generator=g).to(cuda)
    m.train()
    for _ in range(3):  # tracked train steps (no optimizer: the weights stay)
        with torch.autocast("cuda", dtype=BF):
            out = m(torch.randn(32, 3, 32, 32, generator=g).to(cuda))
        F.cross_entropy(out.float(), y).backward()
    assert m._plan.head_on and float((m.conv1[0].running_var - 1).abs().max()) > 1e-2
    R.load_running_stats(m_ref, R.running_stats_state(m))
    m_ref.load_state_dict(m.state_dict())
    for u in (m_ref, m):
        u.eval()
        u.eval_stats = "running"
    m.graph_engine = True
    x = torch.randn(64, 3, 32, 32, generator=g).to(cuda)
    x1 = x[:1].contiguous()

    def run(v):
        with torch.no_grad(), torch.autocast("cuda", dtype=BF):
            return m(v).clone()

    _native.set_deterministic(True)
    try:
        for _ in range(3):  # warm-up, capture + replay, replay
            out = run(x)
            one = run(x1)
        sts = list(m._plan._frozen_graphs.values())
        assert len(sts) == 2 and all(s.stage == "ready" and s.replays == 2 for s in sts) and m._plan.head_on
        assert tuple(out.shape) == (64, 100) and torch.equal(one[0], out[0])
        # a fresh capture under a recording native module and a dispatch log
        m._plan.__dict__.pop("_frozen_graphs")
        real, calls, ops = _native.native(), [], []

        class Recording:
            def __getattr__(self, name):
                fn = getattr(real, name)
                if not callable(fn):
                    return fn

                def wrapped(*a, **kw):
                    calls.append(name)
                    return fn(*a, **kw)
                return wrapped

        class Ops(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                ops.append(func.__name__)
                return func(*args, **(kwargs or {}))

        monkeypatch.setattr(_native, "native", lambda: Recording())
        run(x)
        calls.clear()
        assert torch.equal(run(x), out)  # the capture
        assert calls[-1] == "head_fwd" and calls.count("head_fwd") == 1, calls[-4:]
        calls.clear()
        with Ops():
            again = run(x)  # a bare replay
        assert torch.equal(again, out) and "head_fwd" not in calls
        heads = [o for o in ops if o.split(".")[0] in ("mean", "linear", "addmm", "mm", "matmul", "sum")]
        assert not heads, ops
    finally:
        _native.set_deterministic(False)
    with torch.no_grad():
        out_r = m_ref(x)
        with torch.autocast("cuda", dtype=BF):
            out_rb = m_ref(x)
    e_eng, e_ref = rel(out, out_r), rel(out_rb, out_r)
    print(f"engine {e_eng:.3e} autocast {e_ref:.3e}")
    assert e_eng < max(2.0 * e_ref, 3e-2), (e_eng, e_ref)

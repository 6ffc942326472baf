"""Model definitions: parameter schema (checkpoint compatibility) and forward /
backward numerics against the reference modules (CPU, fp32/fp64)."""
import pytest
import torch
import torch.nn.functional as F

from faster_distributed_training_amd.models import resnet as R
from faster_distributed_training_amd.models import transformer as T
from faster_distributed_training_amd.ops.conv_bn import FusedConvBN2DFunction, conv_bn_reference

from reference_oracle import assert_grads_match, fill_state, golden, golden_json, resnet_batch, schema


def test_resnet50_param_counts():
    m = R.resnet50(10)
    sd = m.state_dict()
    assert len(sd) == 90
    assert sum(p.numel() for p in m.parameters()) == 23_477_194
    assert len(list(m.parameters())) == 69
    assert sd["conv1.0.conv_weight"].shape == (64, 3, 3, 3)
    assert sd["fc.weight"].shape == (10, 2048)
    assert "conv3_x.0.residual_function.3.running_mean" in sd
    assert "conv2_x.0.shortcut.1.num_batches_tracked" in sd


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_resnet_state_dict_matches_reference(arch):
    a = schema(getattr(R, arch)(10).state_dict())
    b = golden_json("state_dict_schema")[arch]
    assert [k for k, _, _ in a] == [k for k, _, _ in b]
    for ea, eb in zip(a, b):
        assert ea == eb  # key, shape and dtype


def test_transformer_state_dict_matches_reference():
    torch.manual_seed(0)
    a = schema(T.Transformer(4, 1000).state_dict())
    b = golden_json("state_dict_schema")["transformer_4_1000"]
    assert [k for k, _, _ in a] == [k for k, _, _ in b]
    for ea, eb in zip(a, b):
        assert ea[1] == eb[1], ea[0]


def test_transformer_param_count():
    m = T.Transformer(4, 30522)
    assert sum(p.numel() for p in m.parameters()) == 29_299_716
    assert len(m.state_dict()) == 105


def test_fused_conv_bn_gradcheck():
    torch.manual_seed(0)
    X = torch.randn(2, 3, 8, 8, dtype=torch.float64, requires_grad=True)
    W = torch.randn(5, 3, 3, 3, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(FusedConvBN2DFunction.apply, (X, W, 1, 1))


def test_fused_conv_bn_matches_reference_function():
    rec = golden("fused_conv_bn")  # the reference's FusedConvBN2DFunction on these inputs
    X, W, g = rec["X"].requires_grad_(), rec["W"].requires_grad_(), rec["g"]
    assert X.shape == (4, 8, 6, 6) and W.shape == (6, 8, 3, 3) and X.dtype == torch.float64
    out_a = conv_bn_reference(X, W, 1, 1, 1e-3)
    gx_a, gw_a = torch.autograd.grad(out_a, (X, W), g)
    out_b, gx_b, gw_b = rec["out"], rec["gx"], rec["gw"]
    assert torch.allclose(out_a, out_b, atol=1e-10)
    assert torch.allclose(gx_a, gx_b, atol=1e-8)
    assert torch.allclose(gw_a, gw_b, atol=1e-8)


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_resnet_forward_backward_matches_reference(arch):
    """Loss and every parameter's gradient against the reference model's on the same seeded
    weights (reference_oracle.fill_state) and batch.  The record keeps a fixed sample of each
    large gradient plus its norm and one dense projection (reference_oracle.grad_record)."""
    rec = golden(f"{arch}_fwd_bwd")
    ma = getattr(R, arch)(10).double()
    fill_state(ma.state_dict(), seed=7)
    ma.fast_path = False
    x, y = resnet_batch()
    la = F.cross_entropy(ma(x), y)
    assert torch.allclose(la, rec["loss"], rtol=1e-9, atol=1e-10)
    la.backward()
    assert len(rec["norm"]) == len(list(ma.parameters()))
    assert_grads_match([(n, p.grad) for n, p in ma.named_parameters()], rec, 1e-6)


def test_flops_per_image():
    m = R.resnet50(10)
    f = R.flops_per_image(m)
    assert abs(f / 2.60e9 - 1) < 0.01


def test_transformer_pieces_match_reference():
    rec = golden("transformer_pieces")  # the reference's LayerNorm / Embeddings on these inputs
    x = rec["x"]
    assert x.shape == (2, 7, 64) and x.dtype == torch.float64
    lna = T.LayerNorm(64).double()
    with torch.no_grad():
        lna.a_2.copy_(rec["ln_a_2"])
    assert torch.allclose(lna(x), rec["ln_out"], atol=1e-10)
    # embeddings (token + position + segment, x sqrt(d))
    ea = T.Embeddings(64, 50, 16).double()
    ea.load_state_dict({k[len("emb."):]: v for k, v in rec.items() if k.startswith("emb.")})
    ids, types = rec["ids"], rec["types"]
    idx = torch.arange(16)
    assert torch.allclose(ea(ids, types, idx), rec["emb_out"].to(torch.float64), atol=1e-6)


def test_fused_mlp_bias_grad_fix_and_faithful():
    torch.manual_seed(0)
    m = T.FusedMLP(8, 16, 4).double()
    x = torch.randn(5, 8, dtype=torch.float64)
    out = m(x)
    ref = F.linear(torch.relu(F.linear(x, m.W1, m.b1[0])), m.W2, m.b2[0])
    assert torch.allclose(out, ref)
    g = torch.randn_like(out)
    out.backward(g)
    gb2 = g.sum(0, keepdim=True)
    assert torch.allclose(m.b2.grad, gb2)
    mf = T.FusedMLP(8, 16, 4, faithful=True).double()
    mf.load_state_dict(m.state_dict())
    mf(x).backward(g)
    assert torch.allclose(mf.b2.grad, gb2 / 5)  # reference averages bias grads (Q5)


def test_transformer_forward_shapes_and_eval_no_mixup():
    torch.manual_seed(0)
    m = T.Transformer(4, 100, n_layers=2, d_model=64, d_ff=128, d_hidden=64, maxlen=32, h=4)
    ids = torch.randint(0, 100, (3, 10))
    types = torch.zeros(3, 10, dtype=torch.long)
    mask = torch.ones(3, 1, 1, 10)
    mask[0, ..., 7:] = 0
    logits, perm, lam = m(ids, types, torch.arange(32), mask)
    assert logits.shape == (3, 4) and perm.shape == (3,)
    m.eval()
    l1, p1, lam1 = m(ids, types, torch.arange(32), mask)
    l2, _, _ = m(ids, types, torch.arange(32), mask)
    assert lam1 == 1.0 and torch.equal(p1, torch.arange(3))
    assert torch.allclose(l1, l2)


def test_attention_masking_is_real():
    from faster_distributed_training_amd.ops.attention import attention_reference
    torch.manual_seed(0)
    q, k, v = (torch.randn(2, 6, 2, 8) for _ in range(3))
    mask = torch.ones(2, 6)
    mask[:, 4:] = 0
    out = attention_reference(q, k, v, mask)
    # changing masked keys/values must not change the output
    k2, v2 = k.clone(), v.clone()
    k2[:, 4:] = 100.0
    v2[:, 4:] = -50.0
    assert torch.allclose(out, attention_reference(q, k2, v2, mask), atol=1e-6)
    # faithful mask value (-1e-9) reproduces the reference bug (no masking)
    a = attention_reference(q, k, v, mask, mask_value=-1e-9)
    assert not torch.allclose(a, attention_reference(q, k2, v2, mask, mask_value=-1e-9))


def test_fused_bias_grad_cpu_path_matches_plain_linear():
    """CPU / plain-PyTorch path of ``bias=`` (ops/dropout._BiasGradTap): a linear called with
    ``bias_grad=False`` feeding dropout_add / gelu_dropout(bias=...) gets the same bias
    gradient as an ordinary linear."""
    import torch.nn.functional as F
    from faster_distributed_training_amd.ops.dropout import dropout_add, gelu_dropout
    from faster_distributed_training_amd.ops.linear import linear
    torch.manual_seed(0)
    h = torch.randn(64, 32, requires_grad=True)
    x = torch.randn(64, 16)
    w = torch.randn(16, 32, requires_grad=True)
    b = torch.randn(16, requires_grad=True)
    g = torch.randn(64, 16)
    for fn in (lambda y, bias: dropout_add(y, x, 0.0, True, None, bias=bias),
               lambda y, bias: gelu_dropout(y, 0.0, True, bias=bias)):
        for t in (h, w, b):
            t.grad = None
        fn(linear(h, w, b, bias_grad=False), b).backward(g)
        got = [t.grad.clone() for t in (h, w, b)]
        for t in (h, w, b):
            t.grad = None
        fn(F.linear(h, w, b), None).backward(g)
        for a, r in zip(got, (h.grad, w.grad, b.grad)):
            torch.testing.assert_close(a, r)


def test_flat_adjacent_scope_keeps_layer_order_for_data_parallel():
    """utils/flat.py adjacency: "shape" (one GPU) moves every same-shape parameter of the model
    next to the first member's slot (the LAST layer with the reversed buffer), "layer" (data
    parallel, world > 1) only each attention block's own Q / K / V -- so the gradient buckets
    still follow the backward's layer order."""
    from faster_distributed_training_amd.models import transformer as T
    from faster_distributed_training_amd.utils.flat import FlatParams
    torch.manual_seed(0)
    m = T.Transformer(4, 1000, n_layers=3, h=4, d_model=64, d_ff=128, d_hidden=64)
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    def layer_of(n):
        for kind in ("sublayer_attention.", "sublayer_ffn."):
            if n.startswith(kind):
                return (kind, int(n[len(kind):].split(".")[0]))
        return None
    lay = FlatParams(m, adjacent="layer")
    order = [s.name for s in lay.slots]
    assert sorted(order) == sorted(names)
    def layer_seq(slots, kind):
        return [layer_of(n)[1] for n in slots if layer_of(n) is not None and layer_of(n)[0] == kind]
    for kind in ("sublayer_attention.", "sublayer_ffn."):
        seq = layer_seq(order, kind)
        assert seq == sorted(seq, reverse=True), "per-layer adjacency keeps the layers in backward order"
    # each block's Q / K / V weights back to back
    for i in range(3):
        qkv = [k for k, n in enumerate(order) if layer_of(n) == ("sublayer_attention.", i) and ".heads." in n
               and n.endswith("weight")]
        assert len(qkv) == 3 and qkv == list(range(qkv[0], qkv[0] + 3))
    shp = layer_seq([s.name for s in FlatParams(m, adjacent="shape").slots], "sublayer_ffn.")
    assert shp != sorted(shp, reverse=True), "shape adjacency groups layers together (single-GPU layout)"

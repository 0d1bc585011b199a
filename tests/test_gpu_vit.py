"""The Point-BERT transformer encoder (mlsp_amd/vit.py on csrc/attn.hip) against the float64 restatement (tests/vit_restatement.py).

Distance: max|a - b| / max|b|.  Yardstick: the distance of the reference's own fp32 result from float64 (the golden for the fixtures,
the restatement run in fp32 on the CPU otherwise).  Floor: the GEMM family's 2e-6 bar (test_gemm_split_bf16_accuracy) per chained
contraction -- a Block chains six (qkv, QK^T, PV, proj, fc1, fc2): 1.2e-5; an encoder of depth D 6 D of them; a functional op alone its
own count.  Bar: max(floor, 3 x yardstick) per quantity -- 3 because the summation order differs.

(The exact gradient of the K third of attn.qkv.bias is 0 -- a softmax does not see a shift common to all keys -- so float64 leaves
~1e-17 there and the relative distance of any fp32 result, the reference's own included, is rounding residue over rounding residue.  The
three thirds of that gradient are measured separately; the K third is held by the same 3 x yardstick rule.)"""
import pytest
import torch

import vit_restatement as vr
from test_vit_cpu import BLOCK_FIXTURE, ENCODER_FIXTURE, load_fixture

pytestmark = pytest.mark.gpu

PER_CONTRACTION = 2e-6
BLOCK_FLOOR = 6 * PER_CONTRACTION


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def make_block(params, heads, dev, **kw):
    from mlsp_amd.vit import Block
    hidden, dim = params["mlp.fc1.weight"].shape
    blk = Block(dim, heads, mlp_ratio=hidden / dim, qkv_bias="attn.qkv.bias" in params, **kw)
    assert blk.mlp.fc1.out_features == hidden
    blk.load_state_dict({n: t.clone() for n, t in params.items()}, strict=True)
    return blk.to(dev)


def make_encoder(params, dim, heads, depth, dev, **kw):
    from mlsp_amd.vit import TransformerEncoder
    hidden = params["blocks.0.mlp.fc1.weight"].shape[0]
    enc = TransformerEncoder(embed_dim=dim, depth=depth, num_heads=heads, mlp_ratio=hidden / dim, qkv_bias="blocks.0.attn.qkv.bias" in params, **kw)
    enc.load_state_dict({n: t.clone() for n, t in params.items()}, strict=True)
    return enc.to(dev)


def param_grads(mod):
    return {n: p.grad.detach().cpu() for n, p in mod.named_parameters()}


def gpu_block_run(params, x, R, heads, dev, masks=None, train=False, **kw):
    """-> (out, grads) on the CPU of one forward + backward of (out * R).sum()"""
    from mlsp_amd.vit import forced_drop_masks
    blk = make_block(params, heads, dev, **kw).train(train)
    xg = x.to(dev).requires_grad_(True)
    if masks is None:
        out = blk(xg)
    else:
        with forced_drop_masks(masks):
            out = blk(xg)
    (out * R.to(dev)).sum().backward()
    grads = param_grads(blk)
    grads["x"] = xg.grad.cpu()
    return out.detach().cpu(), grads


def gpu_encoder_run(params, x, pos, R, R2, heads, depth, dev, masks=None, train=False, **kw):
    from mlsp_amd.vit import forced_drop_masks
    enc = make_encoder(params, x.shape[2], heads, depth, dev, **kw).train(train)
    xg, pg = (t.to(dev).requires_grad_(True) for t in (x, pos))
    if masks is None:
        out, feats = enc(xg, pg)
    else:
        with forced_drop_masks(masks):
            out, feats = enc(xg, pg)
    loss = (out * R.to(dev)).sum()
    for f, r in zip(feats, R2):
        loss = loss + (f * r.to(dev)).sum()
    loss.backward()
    grads = param_grads(enc)
    grads["x"], grads["pos"] = xg.grad.cpu(), pg.grad.cpu()
    return out.detach().cpu(), [f.detach().cpu() for f in feats], grads


def quantities(out, grads, feats=()):
    """name -> tensor, the three thirds of a qkv bias gradient as separate quantities"""
    q = {"out": out}
    for i, f in enumerate(feats):
        q["feat%d" % i] = f
    for n in sorted(grads):
        if n.endswith("attn.qkv.bias"):
            d = grads[n].shape[0] // 3
            for i, third in enumerate("qkv"):
                q["d %s[%s]" % (n, third)] = grads[n][i * d:(i + 1) * d]
        else:
            q["d " + n] = grads[n]
    return q


def check(tag, got, want64, yard, floor):
    """got / want64 / yard: name -> tensor (quantities()); yard is the fp32 reference whose distance from want64 sets the bar"""
    assert sorted(got) == sorted(want64) == sorted(yard), (sorted(got), sorted(want64))
    bad = []
    for name in want64:
        assert torch.isfinite(got[name]).all(), (tag, name)
        assert got[name].shape == want64[name].shape, (tag, name)
        dist, ydist = vr.dist(got[name], want64[name]), vr.dist(yard[name], want64[name])
        bar = max(floor, 3 * ydist)
        print("%s %-34s distance %.3e  yardstick %.3e  bar %.3e" % (tag, name, dist, ydist, bar))
        if not dist <= bar:
            bad.append((name, dist, bar))
    assert not bad, (tag, bad)


def random_block_case(seed, B, L, dim, heads, mlp_ratio=4.0, qkv_bias=True, wscale=1.0):
    g = torch.Generator().manual_seed(seed)
    params = vr.random_block_params(dim, int(dim * mlp_ratio), seed, qkv_bias=qkv_bias, scale=wscale)
    x = torch.randn(B, L, dim, generator=g)
    R = torch.randn(B, L, dim, generator=g)
    return params, x, R


def block_against_float64(tag, params, x, R, heads, dev, scale=None, scales=None, **kw):
    want = quantities(*vr.block_grads(params, x, R, heads, torch.float64, scale, scales))
    yard = quantities(*vr.block_grads(params, x, R, heads, torch.float32, scale, scales))
    out, grads = gpu_block_run(params, x, R, heads, dev, **kw)
    check(tag, quantities(out, grads), want, yard, BLOCK_FLOOR)
    return out, grads


@pytest.fixture(scope="module")
def block_fixture():
    c = load_fixture(BLOCK_FIXTURE)
    heads = int(c["dims"][3])
    c["want"] = quantities(*vr.block_grads(c["params"], c["x"], c["R"], heads, torch.float64))
    return c


@pytest.fixture(scope="module")
def encoder_fixture():
    c = load_fixture(ENCODER_FIXTURE)
    heads, depth = int(c["dims"][3]), int(c["dims"][4])
    out, feats, grads = vr.encoder_grads(c["params"], c["x"], c["pos"], c["R"], [c["R2"]], heads, depth, torch.float64)
    c["want"] = quantities(out, grads, feats)
    return c


def _in_mode(mode, fn):
    from mlsp_amd import functional as Fh
    if mode == "default":
        return fn()
    with Fh.gemm_precision(mode):
        return fn()


@pytest.mark.parametrize("mode", ["default", "fp32"])
def test_block_fixture(dev, block_fixture, mode):
    c = block_fixture
    heads = int(c["dims"][3])
    out, grads = _in_mode(mode, lambda: gpu_block_run(c["params"], c["x"], c["R"], heads, dev))
    check("%s[%s]" % (BLOCK_FIXTURE, mode), quantities(out, grads), c["want"], quantities(c["out"], c["grads"]), BLOCK_FLOOR)


@pytest.mark.parametrize("mode", ["default", "fp32"])
def test_encoder_fixture(dev, encoder_fixture, mode):
    c = encoder_fixture
    heads, depth = int(c["dims"][3]), int(c["dims"][4])
    out, feats, grads = _in_mode(mode, lambda: gpu_encoder_run(c["params"], c["x"], c["pos"], c["R"], [c["R2"]], heads, depth, dev))
    assert len(feats) == 1 and torch.equal(feats[0], out)
    check("%s[%s]" % (ENCODER_FIXTURE, mode), quantities(out, grads, feats), c["want"], quantities(c["out"], c["grads"], [c["feat0"]]),
          6 * depth * PER_CONTRACTION)


@pytest.mark.parametrize("shape", [(1, 1, 8, 2), (3, 2, 16, 4), (2, 65, 384, 6), (1, 67, 36, 1), (1, 256, 64, 1)])
def test_core_edges_against_float64(dev, shape):
    B, L, dim, heads = shape
    params, x, R = random_block_case(sum(shape), B, L, dim, heads)
    out, grads = block_against_float64("shape%s" % (shape,), params, x, R, heads, dev)
    assert out.shape == (B, L, dim)
    if L == 1:                                                               # one token: attention == 1, dS == 0: nothing reaches q or k
        assert not grads["attn.qkv.weight"][:2 * dim].any() and not grads["attn.qkv.bias"][:2 * dim].any()
        assert grads["attn.qkv.weight"][2 * dim:].any()


def test_past_the_lds_limit_raises(dev):
    from mlsp_amd import _lib, functional as Fh
    B, L, dim, heads = 1, 257, 64, 1                                         # L * dh = 16448 > 16384
    params, x, R = random_block_case(9, B, L, dim, heads)
    with pytest.raises(_lib.MlspLibraryError, match="unsupported"):
        gpu_block_run(params, x, R, heads, dev)
    qkv = torch.full((B * L, 3 * dim), 0.5, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(_lib.MlspLibraryError, match="unsupported"):
        Fh.mhsa(qkv, B, L, heads, 0.125)
    for bad in ((1, 513, 4), (1, 4, 132), (1, 8, 6)):                        # L > 512, dh > 128, dh % 4
        with pytest.raises(_lib.MlspLibraryError, match="unsupported"):
            Fh.mhsa(torch.zeros((bad[1], 3 * bad[2]), device=dev), 1, bad[1], 1, 1.0)
    torch.cuda.synchronize()                                                 # nothing was launched: nothing can have faulted


def test_qk_scale_and_mlp_ratio(dev):
    B, L, dim, heads = 2, 21, 32, 4
    params, x, R = random_block_case(31, B, L, dim, heads, mlp_ratio=1.0, qkv_bias=False)
    assert params["mlp.fc1.weight"].shape == (dim, dim)
    block_against_float64("qk_scale", params, x, R, heads, dev, scale=0.37, qk_scale=0.37)


def test_large_logits_stay_finite(dev):
    B, L, dim, heads = 2, 19, 32, 2
    params, x, R = random_block_case(5, B, L, dim, heads)
    params["attn.qkv.weight"] = params["attn.qkv.weight"] * 40.0
    logits = vr.block_forward(params, x, heads, torch.float64, return_logits=True)
    assert float(logits.abs().max()) > 200, float(logits.abs().max())
    assert float(logits.max()) > 200 and float(logits.min()) < -200
    out, grads = block_against_float64("large-logits", params, x, R, heads, dev)
    assert torch.isfinite(out).all() and all(torch.isfinite(g).all() for g in grads.values())


@pytest.mark.parametrize("variant", ["plain", "add", "add+scale", "add-only", "add+scale-only"])
def test_layernorm_alone(dev, variant):
    from mlsp_amd import functional as Fh
    rows_per_sample, B, d = 7, 5, 36
    rows = B * rows_per_sample
    g = torch.Generator().manual_seed(17)
    x, a = torch.randn(rows, d, generator=g) * 3 + 1, torch.randn(rows, d, generator=g)
    w, b = 1 + 0.3 * torch.randn(d, generator=g), 0.2 * torch.randn(d, generator=g)
    Ry, Ru = torch.randn(rows, d, generator=g), torch.randn(rows, d, generator=g)
    s = torch.tensor([1.0, 0.0, 1.25, 1.0, 0.0])
    has_add, has_s, has_ln = "add" in variant, "scale" in variant, "only" not in variant

    def restated(dtype):
        xl, al, wl, bl = (t.detach().to(dtype).requires_grad_(True) for t in (x, a, w, b))
        u = xl
        if has_add:
            u = xl + (al * s.to(dtype)[:, None].repeat_interleave(rows_per_sample, 0) if has_s else al)
        loss = (u * Ru.to(dtype)).sum()
        q = {"u": u.detach()}
        if has_ln:
            y = torch.nn.functional.layer_norm(u, (d,), wl, bl, 1e-5)
            loss = loss + (y * Ry.to(dtype)).sum()
            mean = u.mean(1)
            q.update({"y": y.detach(), "mean": mean.detach(), "rstd": (1 / torch.sqrt(u.var(1, unbiased=False) + 1e-5)).detach()})
        loss.backward()
        q["d x"] = xl.grad
        if has_add:
            q["d add"] = al.grad
        if has_ln:
            q["d weight"], q["d bias"] = wl.grad, bl.grad
        return q
    xg, ag, wg, bg = (t.to(dev).requires_grad_(True) for t in (x, a, w, b))
    u, y, mean, rstd = Fh.layernorm(xg, wg if has_ln else None, bg if has_ln else None, 1e-5, add=ag if has_add else None,
                                    sample_scale=s.to(dev) if has_s else None, rows_per_sample=rows_per_sample if has_s else 0)
    loss = (u * Ru.to(dev)).sum()
    got = {"u": u.detach().cpu()}
    if has_ln:
        assert not mean.requires_grad and not rstd.requires_grad and mean.shape == (rows,)
        loss = loss + (y * Ry.to(dev)).sum()
        got.update({"y": y.detach().cpu(), "mean": mean.cpu(), "rstd": rstd.cpu()})
    else:
        assert y is None and mean is None and rstd is None
    loss.backward()
    got["d x"] = xg.grad.cpu()
    if has_add:
        got["d add"] = ag.grad.cpu()
    if has_ln:
        got["d weight"], got["d bias"] = wg.grad.cpu(), bg.grad.cpu()
    # every scale here but 1.25 is 0 or 1: the sum is exact where torch's own fp32 x + s * a is
    ref = x.to(dev)
    if has_add:
        ref = ref + (a.to(dev) * s.to(dev)[:, None].repeat_interleave(rows_per_sample, 0) if has_s else a.to(dev))
    exact = torch.ones(rows, dtype=torch.bool) if not has_s else ((s == 0) | (s == 1)).repeat_interleave(rows_per_sample)
    assert torch.equal(u.detach().cpu()[exact], ref.cpu()[exact])
    check("layernorm[%s]" % variant, got, restated(torch.float64), restated(torch.float32), PER_CONTRACTION)


def test_gelu_alone(dev):
    from mlsp_amd import functional as Fh
    g = torch.Generator().manual_seed(23)
    x = torch.cat([torch.linspace(-10, 10, 4001)[:4000], torch.rand(1000, generator=g) * 20 - 10, torch.zeros(8)]).view(-1, 8)
    R = torch.randn(x.shape, generator=g)

    def restated(dtype):
        xl = x.to(dtype).requires_grad_(True)
        y = torch.nn.functional.gelu(xl)
        (y * R.to(dtype)).sum().backward()
        return {"y": y.detach(), "d x": xl.grad}
    xg = x.to(dev).requires_grad_(True)
    y = Fh.gelu(xg)
    (y * R.to(dev)).sum().backward()
    check("gelu", {"y": y.detach().cpu(), "d x": xg.grad.cpu()}, restated(torch.float64), restated(torch.float32), PER_CONTRACTION)


def test_mhsa_alone_with_a_wide_row_stride(dev):
    from mlsp_amd import functional as Fh
    B, L, H, dh = 2, 37, 3, 12
    d = H * dh
    g = torch.Generator().manual_seed(29)
    wide = torch.randn(B * L, 3 * d + 8, generator=g)
    R = torch.randn(B * L, d, generator=g)
    scale = 0.21

    def restated(dtype):
        ql = wide[:, :3 * d].to(dtype).requires_grad_(True)
        q, k, v = (ql[:, i * d:(i + 1) * d].reshape(B, L, H, dh).transpose(1, 2) for i in range(3))
        logits = (q @ k.transpose(-1, -2)) * scale
        out = (torch.softmax(logits, -1) @ v).transpose(1, 2).reshape(B * L, d)
        (out * R.to(dtype)).sum().backward()
        return {"out": out.detach(), "lse": torch.logsumexp(logits, -1).detach(), "d qkv": ql.grad}
    wg = wide.to(dev).requires_grad_(True)
    view = wg[:, :3 * d]
    assert view.stride(0) == 3 * d + 8
    out, lse = Fh.mhsa(view, B, L, H, scale)
    assert not lse.requires_grad and lse.shape == (B, H, L)
    (out * R.to(dev)).sum().backward()
    assert not wg.grad[:, 3 * d:].any()
    check("mhsa", {"out": out.detach().cpu(), "lse": lse.cpu(), "d qkv": wg.grad[:, :3 * d].cpu()}, restated(torch.float64),
               restated(torch.float32), 2 * PER_CONTRACTION)


def test_drop_path_eval_equals_rate_zero(dev):
    B, L, dim, heads = 2, 11, 32, 4
    params, x, R = random_block_case(41, B, L, dim, heads)
    a = gpu_block_run(params, x, R, heads, dev, train=False, drop_path=0.3)
    b = gpu_block_run(params, x, R, heads, dev, train=False)
    c = gpu_block_run(params, x, R, heads, dev, train=True)                   # rate 0 in training mode: nn.Identity
    for other in (b, c):
        assert torch.equal(a[0], other[0])
        for n in a[1]:
            assert torch.equal(a[1][n], other[1][n]), n


def test_drop_path_training_with_forced_masks(dev):
    B, L, dim, heads, depth = 3, 10, 32, 4, 2
    rates = [0.2, 0.5]
    g = torch.Generator().manual_seed(43)
    params = {}
    for i in range(depth):
        params.update(vr.random_block_params(dim, 2 * dim, 50 + i, qkv_bias=True, prefix="blocks.%d." % i))
    x, pos, R = torch.randn(B, L, dim, generator=g), 0.5 * torch.randn(B, L, dim, generator=g), torch.randn(B, L, dim, generator=g)
    masks = [torch.tensor(m) for m in ([1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [1.0, 1.0, 0.0], [1.0, 0.0, 0.0])]     # sample 2: always dropped
    scales = [m / (1 - rates[i // 2]) for i, m in enumerate(masks)]
    want = vr.encoder_grads(params, x, pos, R, [], heads, depth, torch.float64, scales=scales)
    yard = vr.encoder_grads(params, x, pos, R, [], heads, depth, torch.float32, scales=scales)
    out, feats, grads = gpu_encoder_run(params, x, pos, R, [], heads, depth, dev, masks=masks, train=True, drop_path_rate=rates)
    assert feats == []
    check("forced-masks", quantities(out, grads), quantities(want[0], want[2]), quantities(yard[0], yard[2]), 6 * depth * PER_CONTRACTION)
    assert torch.equal(out[2], (x[2] + pos[2]) + pos[2])                      # every branch dropped: the rows pass through, plus pos per block
    for n, gr in grads.items():
        if n not in ("x", "pos"):
            assert gr.any(), n
    # a free-running training pass draws its own masks: scales are 0 or 1 / keep_prob per sample
    from mlsp_amd.vit import DropPath, forced_drop_masks
    dp = DropPath(0.5).train()
    s = dp.sample_scale(64, dev)
    assert s.shape == (64,) and set(s.cpu().tolist()) <= {0.0, 2.0}
    with forced_drop_masks([torch.tensor([1.0, 0.0, 1.0])]):                 # the module called on its own scales the samples
        y = dp(x.to(dev))
    assert torch.equal(y.cpu(), x * torch.tensor([2.0, 0.0, 2.0])[:, None, None])


def test_backward_is_bit_reproducible(dev):
    B, L, dim, heads = 2, 33, 48, 4
    params, x, R = random_block_case(11, B, L, dim, heads)
    blk = make_block(params, heads, dev)
    xg = x.to(dev).requires_grad_(True)
    loss = (blk(xg) * R.to(dev)).sum()
    runs = []
    for _ in range(2):                                                       # two backward passes of ONE graph
        blk.zero_grad(set_to_none=True)
        xg.grad = None
        loss.backward(retain_graph=True)
        runs.append(dict(param_grads(blk), x=xg.grad.cpu().clone()))
    for n in runs[0]:
        assert torch.equal(runs[0][n], runs[1][n]), n
    again = gpu_block_run(params, x, R, heads, dev)                          # and a second graph
    for n in runs[0]:
        assert torch.equal(runs[0][n], again[1][n]), n


def test_flat_adam_step_then_second_pass(dev):
    from mlsp_amd.optim import FlatAdam
    B, L, dim, heads = 2, 40, 64, 4
    params, x, R = random_block_case(21, B, L, dim, heads)
    blk = make_block(params, heads, dev)
    opt = FlatAdam(blk.parameters(), lr=1e-3)
    xg, r = x.to(dev), R.to(dev)
    for _ in range(2):
        opt.zero_grad()
        (blk(xg) * r).sum().backward()
        opt.step()
    opt.zero_grad()
    out = blk(xg)                                                            # reads the weight bounds the step kernel published
    (out * r).sum().backward()
    assert torch.isfinite(out).all() and all(p.grad is not None and torch.isfinite(p.grad).all() for p in blk.parameters())
    stepped = {n: t.detach().cpu() for n, t in blk.state_dict().items()}
    assert all(not torch.equal(stepped[n], params[n]) for n in params)
    want = vr.block_forward(stepped, x, heads, torch.float64)
    yard = vr.block_forward(stepped, x, heads, torch.float32)
    dist, bar = vr.dist(out.detach(), want), max(BLOCK_FLOOR, 3 * vr.dist(yard.detach(), want))
    print("after-step out distance %.3e bar %.3e" % (dist, bar))
    assert dist <= bar

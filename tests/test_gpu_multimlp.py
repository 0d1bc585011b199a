"""The heads' merged layers (mlsp_amd/csrc/multi.hip, Fh.multimlp) and the deferred head stack (Fh.pointmlp / Fh.multimlp with
chain=True) against the float64 restatement (tests/multimlp_restatement.py), dropout on.

The reference takes only the GATE PATTERN from the run under test -- which elements are off, and on which side of the activation the
others are -- and computes everything else from the inputs in float64 (multimlp_restatement: z = a * g).  A materialised layer shows
its gate in Z; a deferred layer's activation side is the sign of y * scale + shift of its own pre-BatchNorm output (exact in float64)
and its dropout mask is that of a materialised run with the same dropout stream.  The gate must be ADMISSIBLE (assert_admissible):
its side, or its being off on a channel without dropout, contradicts the sign of the float64 activation only within 1e-5 x max|a| and
on at most 1e-5 of the elements, it is 0 on a channel without dropout only behind a ReLU, holds no value but 0 and the channel's two factors, and keeps the share 1 - t / 256 of the dropout
channels' elements within 5 binomial standard deviations (6 per channel, M >= 256).  tests/test_multimlp_restatement_cpu.py shows that
for these inputs the fp32 restatement's own gate contradicts float64 nowhere.

Distance: max|a - b| / max|b| per quantity.  Yardstick: the same restatement with the same gate in fp32 on the CPU.  Bar:
max(floor, 3 x yardstick) -- 3 because the summation order differs.  Floor: the GEMM family's 2e-6 (test_gemm_split_bf16_accuracy) per
chained contraction: one layer 2e-6 for Z, Y, mean, var and the running statistics, 4e-6 for gradients (forward product + gradient
product); the head stack 8e-6 for everything (four chained forward contractions).  The gradient of a bias in front of a batch-statistics
BatchNorm is exactly zero (float64 leaves ~1e-17 of residue): the kernels write zeros, asserted as such.

Measured on an MI355X, default mode ("f16x3"), as distance / yardstick / bar.  A CONDENSATION: per case only the forward quantity and
the gradient closest to their bars, out of the 10 to 13 quantities of a layer and the 29 of the stack (run with -s for all of them:
every quantity is printed by the tests; the gates had 0 contradictions, but at M = 32768 for 1 of the 2.5e7 elements of the middle layer,
|a64| = 1.4e-8, and in the materialised run for 1 of the 1.7e7 of the last layer, off behind a ReLU without dropout at a64 = +1.8e-7):
  case                               forward                                   gradient
  m33                                var   1.1e-07 / 5.0e-08 / 2.0e-06         dW1        1.6e-07 / 1.3e-07 / 4.0e-06
  m256_mixed                         Y     2.4e-07 / 4.7e-07 / 2.0e-06         dX         2.6e-07 / 4.3e-07 / 4.0e-06
  m256_epilogue                      Y     3.4e-07 / 3.1e-07 / 2.0e-06         dW0        2.2e-07 / 3.3e-07 / 4.0e-06
  m200_epilogue                      Y     3.6e-07 / 3.6e-07 / 2.0e-06         dW2        3.6e-07 / 2.8e-07 / 4.0e-06
  m130_ctot1024                      Y     2.1e-07 / 2.0e-07 / 2.0e-06         dW0        2.8e-07 / 3.1e-07 / 4.0e-06
  model_m1100                        Y     2.0e-07 / 4.7e-07 / 2.0e-06         dW0        2.4e-07 / 2.9e-07 / 4.0e-06
  model_m2048                        Y     2.3e-07 / 5.7e-07 / 2.0e-06         dX         2.5e-07 / 3.5e-07 / 4.0e-06
  m256_mixed_eval                    Y     2.6e-07 / 4.0e-07 / 2.0e-06         dX         2.4e-07 / 2.9e-07 / 4.0e-06
  model_m1100_eval                   Y     2.1e-07 / 4.4e-07 / 2.0e-06         dX         2.5e-07 / 3.7e-07 / 4.0e-06
  m256_shared_input                  Y     2.3e-07 / 5.1e-07 / 2.0e-06         dX         2.2e-07 / 2.8e-07 / 4.0e-06
  m256_overlap_no_dx                 Z     2.4e-07 / 2.8e-07 / 2.0e-06         dW0        3.0e-07 / 3.7e-07 / 4.0e-06
  m256_channel_edges                 Z     2.8e-07 / 4.4e-07 / 2.0e-06         dX         4.3e-07 / 3.4e-07 / 4.0e-06
  stack M = 1100, deferred           out1  2.7e-07 / 2.8e-07 / 8.0e-06         d g1       4.0e-07 / 4.9e-07 / 8.0e-06
  stack M = 1100, materialised       out1  2.7e-07 / 2.8e-07 / 8.0e-06         d g1       4.0e-07 / 4.9e-07 / 8.0e-06
  stack M = 2048, deferred           rm0   4.2e-07 / 3.3e-07 / 8.0e-06         d gb0.beta 4.2e-07 / 4.4e-07 / 8.0e-06
  stack M = 2048, materialised       rm0   4.2e-07 / 3.3e-07 / 8.0e-06         d gb0.beta 4.2e-07 / 4.4e-07 / 8.0e-06
  stack M = 32768, deferred + fused  rm0   8.6e-07 / 3.2e-07 / 8.0e-06         d gb0.beta 2.4e-06 / 9.6e-07 / 8.0e-06
  stack M = 32768, both off          rm0   8.6e-07 / 3.2e-07 / 8.0e-06         d gb0.beta 2.4e-06 / 9.6e-07 / 8.0e-06
  stack M = 32768, loss on head 0    rm0   8.6e-07 / 3.2e-07 / 8.0e-06         d gb0.beta 2.2e-06 / 1.4e-06 / 8.0e-06
  stack M = 32768, loss on heads 0+2 rm0   8.6e-07 / 3.2e-07 / 8.0e-06         d gb0.beta 2.4e-06 / 9.6e-07 / 8.0e-06
"""
import itertools

import pytest
import torch

import multimlp_restatement as mr
from multimlp_restatement import TIER1, ZERO_GAMMA, ZERO_ROW, assert_admissible, case_grads, is_bias_grad, make_case

pytestmark = pytest.mark.gpu

PER_CONTRACTION = 2e-6
LAYER_FWD_FLOOR, LAYER_GRAD_FLOOR, CHAIN_FLOOR = PER_CONTRACTION, 2 * PER_CONTRACTION, 4 * PER_CONTRACTION
MODES = ["default", "fp32"]
TORCH_SEED = 1234


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module", autouse=True)
def drop_the_references_afterwards():
    yield
    for cache in (_KEEPS, _REFS, _PARAMS):
        cache.clear()


def _fh():
    from mlsp_amd import functional as Fh
    return Fh


def precision(mode):
    Fh = _fh()
    return Fh.gemm_precision(Fh.gemm_precision.default if mode == "default" else mode)


def fix_dropout_stream(monkeypatch, counter):
    """the dropout streams are keyed by (torch.initial_seed(), call counter)"""
    torch.manual_seed(TORCH_SEED)
    monkeypatch.setattr(_fh(), "_seed_counter", itertools.count(counter), raising=False)


def check(tag, got, want64, yard, floor_of, exact_zero=()):
    """got / want64 / yard: name -> tensor; floor_of(name) -> floor.  A quantity float64 has as exact zeros must be exact zeros."""
    assert sorted(got) == sorted(want64) == sorted(yard), (sorted(got), sorted(want64))
    bad = []
    for name in want64:
        assert torch.isfinite(got[name]).all(), (tag, name)
        assert got[name].shape == want64[name].shape, (tag, name, got[name].shape, want64[name].shape)
        if name in exact_zero or not want64[name].any():
            nz = int(torch.count_nonzero(got[name]))
            print("%s %-14s exact zeros: %d non-zero" % (tag, name, nz))
            if nz:
                bad.append((name, nz, 0))
            continue
        dist, ydist = mr.dist(got[name], want64[name]), mr.dist(yard[name], want64[name])
        bar = max(floor_of(name), 3 * ydist)
        print("%s %-14s distance %.3e  yardstick %.3e  bar %.3e" % (tag, name, dist, ydist, bar))
        if not dist <= bar:
            bad.append((name, dist, bar))
    assert not bad, (tag, bad)


# ---- tier 1: one multimlp layer, materialised, gate from its own Z ---------------------------------------------------------------------
def layer_floor(name):
    return LAYER_GRAD_FLOOR if name.startswith("d") else LAYER_FWD_FLOOR


def gpu_layer(c, dev, mode, monkeypatch, counter=77):
    """one forward + backward of (Z * R).sum() through Fh.multimlp -> name -> CPU tensor, named as multimlp_restatement.layer_grads"""
    Fh = _fh()
    fix_dropout_stream(monkeypatch, counter)
    X = c["X"].to(dev).requires_grad_(c["x_grad"])
    Ws = [w.to(dev).requires_grad_(True) for w in c["W"]]
    bs = [None if b is None else b.to(dev).requires_grad_(True) for b in c["b"]]
    gamma, beta = (c[k].to(dev).requires_grad_(True) for k in ("gamma", "beta"))
    rm, rv = c["run_mean"].to(dev), c["run_var"].to(dev)
    x_cols = [s[0] for s in c["segs"]]
    with precision(mode):
        assert Fh.multimlp_supported(c["M"], X, Ws, x_cols)
        z = Fh.multimlp(X, list(zip(x_cols, Ws, bs)), gamma, beta, rm, rv, Fh.channel_params(dev, c["spec"]), training=c["training"],
                        p_drop=c["p"])
        assert isinstance(z, torch.Tensor)
        Y, bn_save = z.grad_fn.saved_tensors[1:3]
        (z * c["R"].to(dev)).sum().backward()
    torch.cuda.synchronize()
    q = {"Z": z.detach(), "Y": Y, "mean": bn_save[2], "var": 1.0 / bn_save[3].double() ** 2 - mr.EPS, "run_mean": rm, "run_var": rv,
         "dgamma": gamma.grad, "dbeta": beta.grad}
    if c["x_grad"]:
        q["dX"] = X.grad
    for i, (W, b) in enumerate(zip(Ws, bs)):
        q["dW%d" % i] = W.grad
        if b is not None:
            q["db%d" % i] = b.grad
    return {k: v.detach().cpu() for k, v in q.items()}


def layer_against_float64(name, dev, mode, monkeypatch):
    c = make_case(name)
    got = gpu_layer(c, dev, mode, monkeypatch)
    p = c["p"] if c["training"] else 0.0
    gate = mr.gate_from_z(got["Z"], c["spec"], p)
    tap = []
    want = case_grads(c, gate, torch.float64, tap=tap)
    yard = case_grads(c, gate, torch.float32)
    adm = mr.admissible(gate, tap[0][0], c["spec"], p)
    print(name, mode, adm)
    assert_admissible(adm, c["M"])
    # a bias in front of batch statistics: exact zeros
    zero = [k for k in want if is_bias_grad(k) and c["training"]]
    check("%s %s" % (name, mode), got, want, yard, layer_floor, exact_zero=zero)
    return c, got, gate


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [n for n in sorted(TIER1) if n != "m256_channel_edges"])
def test_one_layer_against_float64(dev, name, mode, monkeypatch):
    c, got, gate = layer_against_float64(name, dev, mode, monkeypatch)
    if not c["training"]:
        # eval: the running statistics are read, not written, and nothing is dropped
        assert torch.equal(got["run_mean"], c["run_mean"]) and torch.equal(got["run_var"], c["run_var"])
        sl, _ = mr.channels(c["spec"])
        assert not (got["Z"][:, sl != 0] == 0).any()


@pytest.mark.parametrize("mode", MODES)
def test_channel_edge_cases(dev, mode, monkeypatch):
    """negative scales, a scale of exactly zero, an all-zero weight row: that column of Y is exactly 0, its variance exactly 0,
    invstd = 1 / sqrt(eps), and Z = act(beta) * g bit for bit"""
    c, got, gate = layer_against_float64("m256_channel_edges", dev, mode, monkeypatch)
    assert torch.isfinite(got["Z"]).all()
    assert not got["Y"][:, ZERO_ROW].any() and got["mean"][ZERO_ROW] == 0
    assert abs(got["var"][ZERO_ROW].item()) <= 4 * 2.0 ** -24 * mr.EPS          # (var read back from the fp32 invstd: its rounding, twice)
    beta = c["beta"][ZERO_ROW]
    assert beta > 0 and torch.equal(got["Z"][:, ZERO_ROW], beta * gate[:, ZERO_ROW].float())
    assert set(gate[:, ZERO_ROW].tolist()) == {0.0, 2.0}
    # gamma == 0: the column is act(beta) wherever it is kept
    b = c["beta"][ZERO_GAMMA]
    sl, _ = mr.channels(c["spec"], torch.float32)
    assert torch.equal(got["Z"][:, ZERO_GAMMA], (b if b > 0 else b * sl[ZERO_GAMMA]) * gate[:, ZERO_GAMMA].float())


def test_partial_overlap_with_an_input_gradient_is_refused(dev, monkeypatch):
    """segments whose input columns overlap in part: the forward is legal (test_one_layer_against_float64[m256_overlap_no_dx]), a
    backward that needs dX fails as unsupported and leaves the device usable.  NOT a launch-free refusal like the four below:
    mlsp_multimlp_bwd_f32 finds the overlap in its per-segment loop, after the reduction and apply passes and segment 0's dgrad and
    weight gradient have been launched; their results are dropped with the exception."""
    from mlsp_amd import _lib
    c = make_case("m256_overlap_no_dx")
    c["x_grad"] = True
    with pytest.raises(_lib.MlspLibraryError, match="unsupported"):
        gpu_layer(c, dev, "default", monkeypatch)
    torch.cuda.synchronize()


REFUSED = {
    "ctot_1028": (256, [(0, 8, 512), (0, 8, 512), (0, 8, 4)]),
    "cout_6": (256, [(0, 8, 6), (8, 8, 6)]),
    "m_32": (32, [(0, 8, 4), (8, 16, 8)]),
    "nine_segments": (256, [(8 * i, 8, 4) for i in range(9)]),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_launch_nothing(dev, name):
    from mlsp_amd import _lib
    Fh = _fh()
    M, segs = REFUSED[name]
    g = torch.Generator().manual_seed(1)
    X = torch.rand(M, max(xc + ci for xc, ci, _ in segs), generator=g).to(dev)
    Ws = [torch.rand(co, ci, generator=g).to(dev).requires_grad_(True) for _, ci, co in segs]
    C = sum(co for _, _, co in segs)
    x_cols = [xc for xc, _, _ in segs]
    torch.cuda.synchronize()
    assert not Fh.multimlp_supported(M, X, Ws, x_cols)
    with pytest.raises(_lib.MlspLibraryError):
        Fh.multimlp(X, [(xc, W, None) for xc, W in zip(x_cols, Ws)], torch.ones(C, device=dev), torch.zeros(C, device=dev),
                    torch.zeros(C, device=dev), torch.ones(C, device=dev), Fh.channel_params(dev, tuple((co, 0.0, False) for _, _, co in segs)))
    torch.cuda.synchronize()


def test_same_dropout_stream_same_bits(dev, monkeypatch):
    c = make_case("model_m1100")
    a = gpu_layer(c, dev, "default", monkeypatch)
    b = gpu_layer(c, dev, "default", monkeypatch)
    assert (a["Z"] == 0).any()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    other = gpu_layer(c, dev, "default", monkeypatch, counter=78)
    assert not torch.equal(other["Z"] == 0, a["Z"] == 0)


# ---- tier 2: the head stack as the model runs it --------------------------------------------------------------------------------------
def gpu_chain(M, dev, mode, defer, fused, weights, monkeypatch, counter=4321):
    """the chain of test_merged_layers_deferred_activation_chain -> (name -> CPU tensor as multimlp_restatement.grads names them,
    per BatchNorm layer what shows its gate: Z, or (y, bn_save) of a DeferredAct; whether each deferred producer's consumers agreed
    to leave its BatchNorm-backward sums)"""
    Fh = _fh()
    fix_dropout_stream(monkeypatch, counter)
    monkeypatch.setattr(Fh, "_DEFER_CHAINS", defer)
    monkeypatch.setattr(Fh, "_FUSE_BWD_STATS", fused)
    params = head_params(M)
    p = {k: (v.to(dev).requires_grad_(True) if k in mr.LEAVES else v.to(dev)) for k, v in params.items()}
    stats = mr.fresh_stats(device=dev)
    shows, agreed = [], []

    def show(h):
        assert isinstance(h, Fh.DeferredAct) == bool(defer)
        shows.append((h.y.detach().cpu(), h.bn_save.cpu()) if defer else h.detach().cpu())
        return h

    def segs(d, table):
        return [(xc, p["%s.W%d" % (d, i)], p.get("%s.b%d" % (d, i))) for i, (xc, _, _, _) in enumerate(table)]
    with precision(mode):
        h1 = show(Fh.pointmlp(p["X"], p["W1"], gamma=p["g1"], beta=p["b1"], run_mean=stats[0], run_var=stats[1], training=True,
                              act=Fh.ACT_RELU, p_drop=mr.P_DROP, chain=True))
        h2 = show(Fh.multimlp(h1, segs("d0", mr.SEG0), p["gb0.gamma"], p["gb0.beta"], stats[2], stats[3], Fh.channel_params(dev, mr.SPEC0),
                              training=True, p_drop=mr.P_DROP, chain=True, spec=mr.SPEC0))
        h3 = show(Fh.multimlp(h2, segs("d1", mr.SEG1), p["gb1.gamma"], p["gb1.beta"], stats[4], stats[5], Fh.channel_params(dev, mr.SPEC1),
                              training=True, p_drop=mr.P_DROP, chain=True, spec=mr.SPEC1))
        slices, cols = Fh.split_columns_shared(h3, [128, 128, 256])
        outs, col = [], 0
        for sl, (_, W, b) in zip(slices, segs("fin", mr.FIN)):
            outs.append(Fh.pointmlp(sl, W, bias=b, training=True, grad_cols=(cols, col)))
            col += sl.shape[1]
        if defer:
            agreed = [h.stats.agreed() for h in (h1, h2, h3)]
        loss = sum(w * (o * p["R%d" % i]).sum() for i, (o, w) in enumerate(zip(outs, weights)) if w)
        loss.backward()
    torch.cuda.synchronize()
    q = {"out%d" % i: o.detach().cpu() for i, o in enumerate(outs)}
    for k in mr.LEAVES:
        q["d " + k] = p[k].grad.cpu() if p[k].grad is not None else torch.zeros_like(params[k])
    q.update(zip(mr.STAT_NAMES, [s.cpu() for s in stats]))
    return q, shows, agreed


_KEEPS = {}      # (M, mode) -> the dropout masks of the materialised run (a hash of the seed and the element index: no values in it)
_REFS = {}       # M -> [(gates, admissibility, {loss weights: (float64 quantities, fp32 quantities)})]: reused while the gates are the same
_PARAMS = {}     # M -> head_params(M) (read only)


def head_params(M):
    for k in [k for k in _PARAMS if k != M]:
        del _PARAMS[k]
    if M not in _PARAMS:
        _PARAMS[M] = mr.head_params(M)
    return _PARAMS[M]


def chain_keeps(M, dev, mode, monkeypatch):
    if (M, mode) not in _KEEPS:
        for k in [k for k in _KEEPS if k[0] != M]:
            del _KEEPS[k]
        _, shows, _ = gpu_chain(M, dev, mode, False, False, (1.0, 1.0, 1.0), monkeypatch)
        _KEEPS[(M, mode)] = [mr.keep_from_z(Z, spec) for Z, spec in zip(shows, mr.SPECS)]
    return _KEEPS[(M, mode)]


def chain_reference(M, gates, weights):
    """-> (float64 quantities, fp32 quantities, admissibility per layer) for this gate set and these loss weights"""
    for k in [k for k in _REFS if k != M]:
        del _REFS[k]
    small = [g.float() for g in gates]
    entry = None
    for e in _REFS.setdefault(M, []):
        if all(torch.equal(a, b) for a, b in zip(e[0], small)):
            entry = e
    if entry is None or weights not in entry[2]:
        tap = []
        want = mr.grads(head_params(M), gates, torch.float64, weights, tap=tap)
        if entry is None:
            entry = (small, [mr.admissible(g, a64, spec, mr.P_DROP) for g, (a64, _), spec in zip(gates, tap, mr.SPECS)], {})
            _REFS[M].append(entry)
        del tap
        entry[2][weights] = (want, mr.grads(head_params(M), gates, torch.float32, weights))
    return entry[2][weights] + (entry[1],)


def chain_against_float64(M, dev, mode, defer, fused, monkeypatch, weights=(1.0, 1.0, 1.0)):
    got, shows, agreed = gpu_chain(M, dev, mode, defer, fused, weights, monkeypatch)
    if defer:
        keeps = chain_keeps(M, dev, mode, monkeypatch)
        gates = [mr.gate_from_preact(y, bn, spec, keep, mr.P_DROP) for (y, bn), spec, keep in zip(shows, mr.SPECS, keeps)]
    else:
        gates = [mr.gate_from_z(Z, spec, mr.P_DROP) for Z, spec in zip(shows, mr.SPECS)]
    del shows
    want, yard, adm = chain_reference(M, gates, weights)
    for a in adm:
        print(M, mode, defer, fused, a)
        assert_admissible(a, M)
    zero = ["d d0.b2", "d d1.b2"]
    check("M=%d %s defer=%d fused=%d %s" % (M, mode, defer, fused, weights), got, want, yard, lambda name: CHAIN_FLOOR, exact_zero=zero)
    return got, agreed


@pytest.mark.parametrize("defer", [False, True])
@pytest.mark.parametrize("mode", ["default", "bf16x6", "fp32"])
@pytest.mark.parametrize("M", [1100, 2048])
def test_head_stack_against_float64(dev, M, mode, defer, monkeypatch):
    chain_against_float64(M, dev, mode, defer, True, monkeypatch)


BS_M = 32768


def smallest_m_with_consumer_side_statistics(mode="bf16x6"):
    """the smallest M, a multiple of 128, at which the dgrads of BOTH merged depths leave their producer's BatchNorm-backward sums"""
    from mlsp_amd import _lib
    lib = _lib.load()

    def parts(M, table, ldx):
        s = (_lib.Seg * len(table))()
        for i, (xc, ci, co, _) in enumerate(table):
            s[i].W, s[i].bias, s[i].ldw, s[i].x_col, s[i].Cin, s[i].Cout = 16, None, ci, xc, ci, co       # (shape query: W is not read)
        return lib.mlsp_multimlp_bwd_stats_parts(M, s, len(table), ldx, ldx, _lib.GEMM_PRECISION_MODES[mode])
    for M in range(128, 4 * BS_M, 128):
        if parts(M, mr.SEG0, 1024) and parts(M, mr.SEG1, 768):
            assert parts(M, mr.SEG0, 1024) == parts(M, mr.SEG1, 768) == M // 128
            return M
    return None


def test_where_the_consumer_side_statistics_start():
    assert smallest_m_with_consumer_side_statistics("bf16x6") == BS_M


@pytest.mark.parametrize("mode,defer,fused", [("default", True, True), ("bf16x6", True, True), ("default", False, False)])
def test_head_stack_consumer_side_statistics(dev, mode, defer, fused, monkeypatch):
    """M = BS_M: the consumers' dgrads store the gradient masked and leave the producers' BatchNorm-backward sums (GemmBs), the producers'
    GEMMs form dY in their operand loads (GemmDy); once more with both switches off.
    Time: BS_M is what the query gives, and at 32768 rows the float64 + fp32 references of one gate set (180 GFLOP each) take 6 to 8 s
    on the CPU, against well under 1 s on the GPU: every case here and below that needs references of its own costs that.  Mode
    "bf16x6" stays because it does not: its gates equal the default mode's, so it reuses their references (1.6 s measured) and is the
    only run of the six-product kernels on the GemmBs / GemmDy path.  Modes "fp32" (no such path) and a second both-off mode are cut."""
    _, agreed = chain_against_float64(BS_M, dev, mode, defer, fused, monkeypatch)
    if defer:
        assert agreed[0] and agreed[1], agreed


@pytest.mark.parametrize("subset", [(0,), (0, 2)])
def test_head_stack_loss_on_a_subset_of_the_heads(dev, subset, monkeypatch):
    """only some of the final layers take part in the backward: the producer gets a masked gradient without complete sums
    (pre_parts = -1); the heads left out get exactly zero weight gradients"""
    weights = tuple(1.0 if i in subset else 0.0 for i in range(3))
    got, agreed = chain_against_float64(BS_M, dev, "default", True, True, monkeypatch, weights)
    assert agreed[0] and agreed[1], agreed
    for i in range(3):
        if i not in subset:
            for k in ["d fin.W%d" % i, "d d1.W%d" % i, "d d0.W%d" % i] + (["d fin.b2"] if i == 2 else []):
                assert not got[k].any(), k

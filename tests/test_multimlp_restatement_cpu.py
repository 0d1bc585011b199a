"""tests/multimlp_restatement.py against torch.nn modules, its gate builders on hand-made inputs, and the inputs of
tests/test_gpu_multimlp.py: for every case there the fp32 restatement's own gate contradicts float64 NOWHERE, so the admissibility
conditions the GPU tests assert are met by the reference alone.  No GPU."""
import pytest
import torch

import multimlp_restatement as mr
from multimlp_restatement import CHAIN_M, TIER1, assert_admissible, case_grads, is_bias_grad, make_case, random_keep


# ---- the restatement against torch.nn ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("name", ["m33", "m256_mixed", "m200_epilogue", "m256_shared_input", "m256_channel_edges"])
def test_layer_equals_nn_modules(name, training):
    c = make_case(name)
    X = c["X"].double()
    outs, rms, rvs, col = [], [], [], 0
    for (xc, ci, co, hb, sl, _), W, b in zip(c["segs"], c["W"], c["b"]):
        lin = torch.nn.Linear(ci, co, bias=hb).double()
        bn = torch.nn.BatchNorm1d(co, eps=mr.EPS, momentum=0.1).double()
        act = torch.nn.Identity() if sl == 1.0 else torch.nn.ReLU() if sl == 0.0 else torch.nn.LeakyReLU(sl)
        with torch.no_grad():
            lin.weight.copy_(W)
            if hb:
                lin.bias.copy_(b)
            bn.weight.copy_(c["gamma"][col:col + co]); bn.bias.copy_(c["beta"][col:col + co])
            bn.running_mean.copy_(c["run_mean"][col:col + co]); bn.running_var.copy_(c["run_var"][col:col + co])
        mods = torch.nn.Sequential(lin, bn, act).train(training)
        outs.append(mods(X[:, xc:xc + ci]).detach())
        rms.append(bn.running_mean); rvs.append(bn.running_var)
        col += co
    z, y, mean, var, rm, rv = mr.layer(X, c["rs_segs"], c["gamma"], c["beta"], c["run_mean"], c["run_var"],
                                       lambda a: mr.act_gate(a, c["spec"]), training)
    assert mr.dist(z, torch.cat(outs, 1)) <= 1e-12
    assert mr.dist(rm, torch.cat(rms)) <= 1e-12 and mr.dist(rv, torch.cat(rvs)) <= 1e-12
    if training:
        assert mr.dist(mean, y.mean(0)) <= 1e-12 and mr.dist(var, y.var(0, unbiased=False)) <= 1e-12
    else:
        assert torch.equal(rm, c["run_mean"].double()) and torch.equal(rv, c["run_var"].double())


@pytest.mark.parametrize("p", [0.5, 0.3])
def test_layer_with_an_explicit_keep_mask(p):
    c = make_case("m256_epilogue")
    sl, dr = mr.channels(c["spec"])
    keep = random_keep(c["R"].shape, p, 3)
    z, y, mean, var, _, _ = mr.layer(c["X"], c["rs_segs"], c["gamma"], c["beta"], None, None, lambda a: mr.act_gate(a, c["spec"], keep, p))
    bn = c["gamma"].double() * (y - mean) / torch.sqrt(var + mr.EPS) + c["beta"].double()
    act = torch.where(bn > 0, bn, bn * sl)
    want = torch.where(dr, act * keep * mr.inv_keep(p), act)
    assert mr.dist(z, want) <= 1e-14
    assert (z[:, ~dr] != 0).all() and ((z == 0) | keep)[:, dr].all()


def test_inv_keep_is_the_byte_threshold_contract():
    assert mr.inv_keep(0.3) == 256 / 179 and mr.thresh(0.3) == 77
    assert mr.inv_keep(0.5) == 2 and mr.thresh(0.5) == 128
    assert mr.inv_keep(0.0) == 1 and mr.thresh(0.0) == 0
    assert mr.thresh(0.999) == 255 and mr.inv_keep(0.999) == 256


# ---- the gate builders on hand-made inputs --------------------------------------------------------------------------------------------
SPEC4 = ((1, 0.0, True), (1, 0.2, True), (1, 1.0, True), (1, 0.0, False), (1, 0.2, False), (1, 1.0, False))


def test_gate_from_z_by_hand():
    ik = 256 / 179
    Z = torch.tensor([[1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
                      [0.0, -1.0, -1.0, 0.0, -1.0, -1.0],          # ReLU-off (under dropout: or dropped), negative sides
                      [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],              # exact zeros: off where dropout or ReLU may be the cause; else a == 0
                      [2e-30, -2e-31, -1e-30, 1e-30, -2e-31, -1e-30]])
    g = mr.gate_from_z(Z, SPEC4, 0.3)
    want = torch.tensor([[ik, ik, ik, 1, 1, 1],
                         [0, 0.2 * ik, ik, 0, 0.2, 1],
                         [0, 0, 0, 0, 0.2, 1],
                         [ik, 0.2 * ik, ik, 1, 0.2, 1]], dtype=torch.float64)
    assert torch.equal(g, want)
    keep = mr.keep_from_z(Z, SPEC4)
    assert keep.tolist() == [[True] * 6, [False, True, True, True, True, True], [False, False, False, True, True, True], [True] * 6]
    # eval / p = 0: no dropout channel is left
    assert torch.equal(mr.gate_from_z(Z, SPEC4, 0.0)[2], torch.tensor([0, 0.2, 1, 0, 0.2, 1], dtype=torch.float64))


def test_gate_from_preact_by_hand():
    ik = 2.0
    # a = y * scale + shift: tiny pre-activations keep their sign in float64 (1e-30 * 1 + 0; 3 * (1/3 in fp32) - 1 > 0 by one fp32 ulp / 3)
    third = torch.tensor(1.0 / 3.0, dtype=torch.float32).item()
    y = torch.tensor([[1e-30, -1e-30, -1e-30, 3.0, -3.0, 0.0],
                      [-1e-30, 1e-30, 1e-30, -1e-30, 1e-30, -1e-30]], dtype=torch.float32)
    bn = torch.zeros(4, 6)
    bn[0] = torch.tensor([1.0, 1.0, -1.0, third, third, 1.0])
    bn[1] = torch.tensor([0.0, 0.0, 0.0, -1.0, 1.0, 0.0])
    keep = torch.tensor([[True, True, False, True, True, True], [True, False, True, False, False, False]])
    g = mr.gate_from_preact(y, bn, SPEC4, keep, 0.5)
    a3 = 3.0 * third - 1.0
    assert a3 != 0 and abs(a3) < 1e-7
    want = torch.tensor([[ik, 0.2 * ik, 0, 1 if a3 > 0 else 0, 1 if -a3 > 0 else 0.2, 1],
                         [0, 0, ik, 0, 1, 1]], dtype=torch.float64)
    assert torch.equal(g, want)
    assert torch.equal(mr.gate_from_preact(y, bn, SPEC4, None, 0.0)[1], torch.tensor([0, 1, 1, 0, 1, 1], dtype=torch.float64))


def test_admissible_counts_by_hand():
    a64 = torch.tensor([[1.0, -1.0, 1.0, 1.0, -1.0, 1.0], [1.0, 1.0, -1.0, -1.0, 1.0, -1.0]], dtype=torch.float64)
    good = mr.act_gate(a64, SPEC4, torch.tensor([[True] * 6, [False] * 6]), 0.5)
    a = mr.admissible(good, a64, SPEC4, 0.5)
    assert (a["bad_values"], a["illegal_off"], a["contradictions"], a["contra_max"]) == (0, 0, 0, 0.0)
    assert (a["eligible"], a["kept"]) == (6, 3) and a["keep_sigma"] == 0 and a["tau"] == 1e-5
    bad = good.clone()
    bad[0, 0] = 0.4          # ReLU + dropout channel, positive: the negative side's factor of ANOTHER channel
    bad[0, 3] = 2.0          # a channel without dropout carries the dropout factor
    bad[0, 4] = 0.0          # LeakyReLU without dropout switched off
    bad[1, 1] = 0.4          # on with the negative side where a64 > 0
    bad[1, 4] = 0.2          # the same on a channel without dropout
    a = mr.admissible(bad, a64, SPEC4, 0.5)
    assert (a["bad_values"], a["illegal_off"], a["contradictions"], a["contra_max"]) == (2, 1, 2, 1.0)
    # OFF where float64 is positive, on a channel without dropout: a contradiction behind a ReLU too (nothing but a non-positive
    # activation switches such an element off), and no contradiction on the dropout channel beside it
    spec = ((2, 0.0, False), (2, 0.0, True))
    a64 = torch.tensor([[1.0, -1.0, 1.0, -1.0], [3.0, 2e-5, 3.0, 1.0]], dtype=torch.float64)
    gate = mr.gate_from_z(torch.tensor([[0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 2.0]]), spec, 0.5)
    a = mr.admissible(gate, a64, spec, 0.5)
    assert (a["bad_values"], a["illegal_off"], a["contradictions"], a["contra_max"]) == (0, 0, 3, 3.0) and a["tau"] == pytest.approx(3e-5)
    with pytest.raises(AssertionError):
        assert_admissible(a, 2)


# ---- the inputs of the GPU tests: the fp32 gate is the float64 gate -------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(TIER1))
def test_tier1_inputs_leave_no_sign_to_chance(name):
    c = make_case(name)
    p = c["p"] if c["training"] else 0.0
    keep = random_keep(c["R"].shape, p, c["seed"]) if p else None
    t32, t64 = [], []
    q32 = case_grads(c, lambda a: mr.act_gate(a, c["spec"], keep, p), torch.float32, tap=t32)
    gate = mr.gate_from_z(q32["Z"], c["spec"], p)
    assert torch.equal(mr.gate_from_z(q32["Z"], c["spec"], p, torch.float32), t32[0][1])         # what Z shows is the gate that made it
    q64 = case_grads(c, gate, torch.float64, tap=t64)
    assert_admissible(mr.admissible(gate, t64[0][0], c["spec"], p), c["M"], zero_contradictions=True)
    for k in q64:
        if not (is_bias_grad(k) and c["training"]):          # (in front of batch statistics: rounding residue over rounding residue)
            assert mr.dist(q32[k], q64[k]) <= 2e-6, (k, mr.dist(q32[k], q64[k]))


@pytest.mark.parametrize("M", CHAIN_M)
def test_chain_inputs_leave_no_sign_to_chance(M):
    params = mr.head_params(M)
    keeps = [random_keep((M, sum(c for c, _, _ in spec)), mr.P_DROP, 30 + i) for i, spec in enumerate(mr.SPECS)]
    t32, t64 = [], []
    q32 = mr.grads(params, [lambda a, s=spec, k=keep: mr.act_gate(a, s, k, mr.P_DROP) for spec, keep in zip(mr.SPECS, keeps)], torch.float32, tap=t32)
    gates = [mr.act_gate(a32.double(), spec, keep, mr.P_DROP) for (a32, _), spec, keep in zip(t32, mr.SPECS, keeps)]
    q64 = mr.grads(params, gates, torch.float64, tap=t64)
    for gate, (a64, _), spec in zip(gates, t64, mr.SPECS):
        assert_admissible(mr.admissible(gate, a64, spec, mr.P_DROP), M, zero_contradictions=True)
    for k in q64:
        if k not in ("d d0.b2", "d d1.b2"):
            assert mr.dist(q32[k], q64[k]) <= 8e-6, (k, mr.dist(q32[k], q64[k]))


# ---- the floors of the GPU tests against the mistakes a self-comparison cannot see -----------------------------------------------------
def test_the_floors_see_a_wrong_rescale_a_shifted_switch_and_a_biased_running_variance():
    """what each mistake moves in float64, against the 2e-6 / 4e-6 floors of tests/test_gpu_multimlp.py (the yardsticks above are below
    1e-6, so the floors are the bars): survivors rescaled by 1 / (1 - p) where the kernels' contract is 256 / (256 - t); the per-channel
    slope and dropout switch one quad off; the running variance fed the biased batch variance"""
    c = make_case("model_m1100")
    p, M = c["p"], c["M"]
    keep = random_keep(c["R"].shape, p, 5)
    right = case_grads(c, lambda a: mr.act_gate(a, c["spec"], keep, p), torch.float64)

    def moved(q, names):
        return min(mr.dist(q[k], right[k]) for k in names)
    grads = [k for k in right if k.startswith("d") and not is_bias_grad(k)]
    rescale = case_grads(c, lambda a: mr.act_gate(a, c["spec"], keep, p) * ((1 / (1 - p)) / mr.inv_keep(p)), torch.float64)
    assert moved(rescale, ["Z"] + grads) > 1e-3 * 0.99
    (c0, s0, d0), (c1, s1, d1), (c2, s2, d2) = c["spec"]
    off = ((c0, s0, d0), (c1 + 4, s1, d1), (c2 - 4, s2, d2))
    shifted = case_grads(c, lambda a: mr.act_gate(a, off, keep, p), torch.float64)
    assert moved(shifted, ["Z", "dX", "dW2", "dgamma", "dbeta"]) > 1e-3
    biased = 0.9 * c["run_var"].double() + 0.1 * right["var"]
    assert mr.dist(biased, right["run_var"]) > 10 * 2e-6

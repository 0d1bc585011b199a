"""The generated K-tile bodies of gemm_split_kernel (mlsp_amd/csrc/gen_split_body.py; the text is a build product and is not committed).
Whatever the placement, a body must issue every piece product once, pin every slot, write every image plane of every staged quad once,
reload a quad only after its last use, transform exactly the operand its variant names, and -- the f16 bodies -- touch no image before the
mid-body barrier.  The statements are matched as text; no compiler and no GPU."""
import collections
import importlib.util
import os
import re

import pytest

_spec = importlib.util.spec_from_file_location(
    "gen_split_body", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mlsp_amd", "csrc", "gen_split_body.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

COMBOS = [(wm, v, npc == 2) for (npc, _dy, _xf, _xd), v in gen.VARIANTS.items() for wm in (1, 2)]

SCHED = "__builtin_amdgcn_sched_barrier(0);"
MFMA = re.compile(r"acc\[(\d)\]\[(\d)\] = __builtin_amdgcn_mfma_f32_32x32x16_(bf16|f16)\((SXH\()?a\[(\d)\]\[(\d)\]\[(\d)\]\)?, (?:SXH\()?"
                  r"b\[(\d)\]\[(\d)\]\[(\d)\]\)?, acc\[(\d)\]\[(\d)\], 0, 0, 0\);")
WRITE = re.compile(r"\*\(u32x2\*\)\(w([ab]) \+ (\d) \* WQ([AB]) \+ (\d) \* SX_PLANE\) = \(u32x2\)\{\S+\[0\], \S+\[1\]\};")
LOAD = re.compile(r"raw\[(\d)\] = SX_LOAD_([AB])\((\d)\);")
DY_LOAD = re.compile(r"SX_DY_LOAD\((\d)\);")
DY_A = re.compile(r"SX_DY_A\((\d), ([01])\);")
XF = re.compile(r"SX_XF_([AB])\((\d), ([01])\);")
XF_HASH = re.compile(r"SX_XF_HASH_([AB])\((\d)\);")
SPLIT = re.compile(r"(pk[012]\[[01]\]|pkd\[\d\]\[[01]\]\[[01]\]|r0|r1|a1) = [^;]+;")       # the split arithmetic: registers only


def check_body(lines, wm, variant, half):
    st = [s for s in lines if not s.startswith("//")]
    nqa, npc = 2 * wm, 2 if half else 3
    quad = lambda op, q: q if op == "A" else nqa + q            # index into raw[] of an operand's quad
    at = collections.defaultdict(list)                           # (kind, ...) -> statement indices
    for n, s in enumerate(st):
        if s == SCHED:
            at["sched",].append(n)
        elif s.startswith("__syncthreads();"):
            at["sync",].append(n)
        elif m := MFMA.fullmatch(s):
            i, j, kind, sxh, s2, ai, pa, s2b, bj, pb, i2, j2 = m.groups()
            assert (i, j, s2) == (i2, j2, s2b) and (ai, bj) == (i, j), s
            assert (kind == "f16") == half == bool(sxh), s
            at["mfma",].append(n)
            at["product", int(s2), int(i), int(j), int(pa), int(pb)].append(n)
        elif m := WRITE.fullmatch(s):
            w, q, wq, plane = m.groups()
            assert w.upper() == wq, s
            qd = int(q) if wq == "A" else nqa + int(q)           # (wa is indexed by the quad, wb by the B quad)
            at["write",].append(n)
            at["write", qd, int(plane)].append(n)
        elif m := LOAD.fullmatch(s):
            qd, op, q = m.groups()
            assert int(qd) == quad(op, int(q)), s
            at["load", int(qd)].append(n)
        elif m := DY_LOAD.fullmatch(s):
            at["dy_load", int(m[1])].append(n)
        elif m := DY_A.fullmatch(s):
            at["dy_a", int(m[1]), int(m[2])].append(n)
            at["use", int(m[1])].append(n)
        elif m := XF.fullmatch(s):
            at["xf", m[1], int(m[2]), int(m[3])].append(n)
            at["use", quad(m[1], int(m[2]))].append(n)
        elif m := XF_HASH.fullmatch(s):
            at["xf_hash", m[1], int(m[2])].append(n)
        else:
            assert SPLIT.fullmatch(s), "unknown statement: " + s
            for qd, e in re.findall(r"raw\[(\d)\]\[(\d)\]", s):
                at["use", int(qd)].append(n)
                at["convert", int(qd), int(e) // 2].append(n)
    keys = lambda kind: sorted(k[1:] for k in at if k[0] == kind and len(k) > 1)
    once = lambda *k: (at[k][0] if len(at[k]) == 1 else pytest.fail("%r: %d times" % (k, len(at[k]))))

    # every piece product of every (k16 step, row window, column window) once, nothing else
    QA, QB = gen.pieces(half)
    assert len(QA) == (3 if half else 6) and len(at["mfma",]) == 4 * len(QA) * wm
    assert keys("product") == sorted((s2, i, j, pa, pb) for s2 in range(2) for i in range(wm) for j in range(2) for pa, pb in zip(QA, QB))
    assert all(len(at[("product",) + k]) == 1 for k in keys("product"))
    # every MFMA closes its slot with exactly one sched_barrier(0) before the next MFMA
    for n, nxt in zip(at["mfma",], at["mfma",][1:] + [len(st)]):
        assert len([b for b in at["sched",] if n < b < nxt]) == 1, st[n]
    assert len(at["sched",]) == len(at["mfma",]) and at["mfma",][0] == 0

    # staging: each quad's planes written once, the quad reloaded once and only after its last use
    assert keys("write") == [(qd, p) for qd in range(nqa + 4) for p in range(npc)]
    assert keys("load") == [(qd,) for qd in range(nqa + 4)]
    for qd in range(nqa + 4):
        for p in range(npc):
            once("write", qd, p)
        assert once("load", qd) > max(at["use", qd]), qd
        for hh in range(2):
            assert at["convert", qd, hh], (qd, hh)
    dy = variant.startswith("dy")
    assert keys("dy_load") == ([(q,) for q in range(nqa)] if dy else [])
    assert keys("dy_a") == ([(q, hh) for q in range(nqa) for hh in range(2)] if dy else [])
    for q, hh in keys("dy_a"):
        once("dy_load", q)
        assert once("dy_a", q, hh) < min(at["convert", q, hh]), (q, hh)

    # transforms: on the operand the variant names and on no other; the quad's hash first
    op = "A" if variant.startswith("xa") else "B" if "xb" in variant else None
    nq = {"A": nqa, "B": 4, None: 0}[op]
    assert keys("xf") == [(op, q, hh) for q in range(nq) for hh in range(2)]
    assert keys("xf_hash") == ([(op, q) for q in range(nq)] if variant.endswith("d") else [])
    for _, q, hh in keys("xf"):
        assert once("xf", op, q, hh) < min(at["convert", quad(op, q), hh]), (q, hh)
        if variant.endswith("d"):
            assert once("xf_hash", op, q) < at["xf", op, q, hh][0], (q, hh)

    # f16: one barrier between the two k16 steps, and no image write while another wave may still read the images
    if half:
        sync = once("sync",)
        step = {n: k[1] for k in at if k[0] == "product" for n in at[k]}
        assert all((n > sync) == (step[n] == 1) for n in at["mfma",])
        assert min(at["write",]) > sync, st[min(at["write",])]
    else:
        assert not at["sync",]


@pytest.mark.parametrize("wm,variant,half", COMBOS, ids=["%swm%d%s" % ("h_" if h else "", w, "_" + v if v else "") for w, v, h in COMBOS])
def test_body(wm, variant, half):
    check_body(gen.body(wm, variant, half), wm, variant, half)


def test_variant_table():
    assert len(COMBOS) == len(set(COMBOS)) == 32
    assert {k[0] for k in gen.VARIANTS} == {2, 3}


def test_ladder_names_each_table_entry_once(tmp_path):
    """the generated file: one `if constexpr` branch per VARIANTS row, holding that row's body for WM == 2 and for WM == 1"""
    path = tmp_path / "gemm_split_body.inc"
    gen.main(str(path))
    lines = path.read_text().split("\n")
    cond = re.compile(r"(?:\} else )?if constexpr \(NPC == (\d) && DY == (true|false) && XF == (\d) && XD == (true|false)\) \{")
    heads = [(n, m) for n, s in enumerate(lines) if (m := cond.fullmatch(s))]
    assert [(int(m[1]), m[2] == "true", int(m[3]), m[4] == "true") for _, m in heads] == list(gen.VARIANTS)
    assert sum("if constexpr" in s for s in lines) == len(heads) and heads[0][0] == 0
    ends = [n for n, _ in heads[1:]] + [len(lines) - 2]
    assert lines[-2].startswith("} else static_assert(") and lines[-1] == ""
    for (n, m), end, (key, v) in zip(heads, ends, gen.VARIANTS.items()):
        seg = lines[n + 1:end]
        b2, b1 = gen.body(2, v, key[0] == 2), gen.body(1, v, key[0] == 2)
        assert len(seg) == len(b2) + len(b1) + 3
        assert seg[0].startswith("if (WM == 2) {") and seg[1:1 + len(b2)] == b2
        assert seg[1 + len(b2)].startswith("} else {") and seg[2 + len(b2):-1] == b1 and seg[-1] == "}"

#!/usr/bin/env python3
"""Emits the hand-placed K-tile bodies of gemm_split_kernel (gemm.hip): straight-line code, one MFMA per issue slot with its fillers, every
slot closed by sched_barrier(0) so the compiler keeps the placement.

    python3 gen_split_body.py build/gemm_split_body.inc

writes the one file the kernel includes: the `if constexpr` ladder over VARIANTS with body(wm, variant, half) in place for both tile
heights (WM = 2: 128 x 128 tile, 1: 64 x 128).  The file is a build product; tests/test_split_body_cpu.py checks every body.

Per K-tile (32 deep) a wave issues 24 * WM MFMAs (2 k16 steps x WM x 2 accumulators x 6 piece products).  The MFMA shadow is 32 cycles = 8
issue slots of 4; between two MFMAs sits vector work of the NEXT tile's staging: per staged quad (16-byte load) two element pairs x three
micro-steps of the three-way bf16 split, then its three image writes and the global load of the quad after next.

VARIANT (operand transform instantiations, gemm_split_kernel<.., XF, XD, DY>): dy / dyxb / dyxbd = the A quads are (d', y) pairs turned into
the layer's output gradient (SX_DY_A) [+ the xb / xbd transform on B]; xa / xad = the A quads are transformed before their split
(SX_XF_A: scale * x + shift, activation as one max; `d`: + dropout, one hash per quad), xb / xbd = the same on the B quads (SX_XF_B).
The transform roughly doubles the vector work of the quads it applies to; placing it with the split steps of those quads overflows the MFMA
shadow of a third of the slots (measured: +27 % per launch).  In the variants the work items keep their ORDER but are spread over the slots
by WEIGHT (approximate vector instructions), so every slot carries the same load whichever operand is transformed.
The plain body (no VARIANT) is the round-3 placement, unchanged: its 3 * 2 * (NQA + 4) micro-steps spread evenly BY COUNT (one per slot at
WM = 2, one or two at WM = 1).

HALF (two f16 pieces, three products: gemm_split_kernel<.., NPC = 2>): the K-tile body is cut in two phases by a barrier.  The fragments of
BOTH k16 steps are requested before the body; phase 1 (the MFMAs of step 0) only waits for step 0's and stages the first Q1 quads in
registers while step 1's fragments arrive; at the barrier every wave holds all its fragments, and phase 2 (the MFMAs of step 1) writes the
images -- the deferred quads' first.  (Before: all 16 fragment reads were waited for in front of the first MFMA.)  Each phase spreads its
items by weight over its own half of the slots.

Names used: acc, a[s2][i][q], b[s2][j][q], raw[8], pk0/pk1/pk2[2], pkd, r0, r1, a1, wa, wb, WQA, WQB, SX_LOAD_A/B, SX_XF_A/B, SX_XF_HASH_A/B,
SX_DY_A, SX_DY_LOAD (see the kernel)."""
import sys

# gemm_split_kernel<.., XF, XD, DY, NPC>: (NPC, DY, XF, XD) -> VARIANT, each for WM = 2 and 1.  The one table of the instantiations that
# exist (launch_gemm's SPLIT_*_GO); the kernel's ladder is emitted from it and an instantiation outside it does not compile.
VARIANTS = {(npc, dy, xf, xd): v for npc in (2, 3) for (dy, xf, xd), v in {
    (True, 0, False): "dy", (True, 2, False): "dyxb", (True, 2, True): "dyxbd", (False, 0, False): "",
    (False, 1, False): "xa", (False, 1, True): "xad", (False, 2, False): "xb", (False, 2, True): "xbd"}.items()}


def pieces(half):
    """(QA, QB): the A / B piece of each product, smallest products first, the leading one last"""
    return ([1, 0, 0], [0, 1, 0]) if half else ([1, 0, 2, 0, 1, 0], [1, 2, 0, 1, 0, 0])


def items(wm, variant, half):
    """ordered work items (weight, [statements]) of one K-tile's staging: those of phase 1 (HALF only), then all the others"""
    NQA = 2 * wm                      # A quads of a tile per thread (B: 4)
    DYA = variant.startswith("dy")    # dy / dyxb / dyxbd: the A quads are d' + y pairs (SX_DY_A: the BatchNorm backward, 3 operations per value; SX_DY_LOAD)
    XA = variant.startswith("xa")
    XB = variant.startswith("xb") or variant.startswith("dyxb")
    DROP = variant.endswith("d")
    Q1 = (3 * (NQA + 4) + 4) // 5 if half else 0
    early, writes, rest = [], [], []
    for qd in range(NQA + 4):
        isA = qd < NQA
        xf = (XA and isA) or (XB and not isA)
        q = qd if isA else qd - NQA
        op = "A" if isA else "B"
        out = early if qd < Q1 else rest
        if xf and DROP:
            out.append((10, [f"SX_XF_HASH_{op}({q});"]))
        for hh in range(2):
            x0, x1 = f"raw[{qd}][{2 * hh}]", f"raw[{qd}][{2 * hh + 1}]"
            if DYA and isA:
                out.append((6, [f"SX_DY_A({q}, {hh});"]))
            if xf:
                out.append((10 if DROP else 6, [f"SX_XF_{op}({q}, {hh});"]))
            if half:
                # x * s = h0 + h1 (+ < 2^-22 |x s|): h0 = f16(x s), h1 = f16(x s - h0) (the remainder is exact in fp32); s: the operand's
                # power-of-two scale (sxs_a / sxs_b).  Per pair: v_pk_mul (or 2 v_mul), v_cvt_pk_f16_f32, 2 v_fma_mix_f32 (x s - h0, reading the f16
                # half in place), v_cvt_pk_f16_f32
                sc = "sxs_a" if isA else "sxs_b"
                # quads staged in phase 1 keep their pieces in pkd[qd] and are written to the images in phase 2; the others use the
                # scratch pair pk0 / pk1 and are written at once
                P0, P1 = (f"pkd[{qd}][0]", f"pkd[{qd}][1]") if qd < Q1 else ("pk0", "pk1")
                out.append((3, [f"{P0}[{hh}] = sx_cvt_pk_h({x0} * {sc}, {x1} * {sc});"]))
                L = [f"{P1}[{hh}] = sx_cvt_pk_h(sx_rem_lo({x0}, {sc}, {P0}[{hh}]), sx_rem_hi({x1}, {sc}, {P0}[{hh}]));"]
                w = 3
                if hh == 1:
                    d = f"wa + {qd} * WQA" if isA else f"wb + {q} * WQB"
                    W = [f"*(u32x2*)({d} + {p} * SX_PLANE) = (u32x2){{{(P0, P1)[p]}[0], {(P0, P1)[p]}[1]}};" for p in range(2)]
                    if qd < Q1:
                        writes.append((2, W))
                    else:
                        L += W
                        w += 2
                    L.append(f"raw[{qd}] = SX_LOAD_{op}({q});")
                    if DYA and isA:
                        L.append(f"SX_DY_LOAD({q});")
                    w += 1
                out.append((w, L))
                continue
            out.append((4, [f"pk0[{hh}] = sx_cvt_pk({x0}, {x1});", f"a1 = __uint_as_float(pk0[{hh}] & 0xffff0000u);",
                            f"r0 = {x0} - __uint_as_float(pk0[{hh}] << 16);"]))
            out.append((2, [f"r1 = {x1} - a1;", f"pk1[{hh}] = sx_cvt_pk(r0, r1);"]))
            L = [f"pk2[{hh}] = sx_cvt_pk(r0 - __uint_as_float(pk1[{hh}] << 16), r1 - __uint_as_float(pk1[{hh}] & 0xffff0000u));"]
            w = 5
            if hh == 1:
                d = f"wa + {qd} * WQA" if isA else f"wb + {q} * WQB"
                for p in range(3):
                    L.append(f"*(u32x2*)({d} + {p} * SX_PLANE) = (u32x2){{pk{p}[0], pk{p}[1]}};")
                L.append(f"raw[{qd}] = SX_LOAD_{op}({q});")
                if DYA and isA:
                    L.append(f"SX_DY_LOAD({q});")
                w += 4
            out.append((w, L))
    return early, writes + rest


def mfma(c, wm, half):
    QA, QB = pieces(half)
    s2, rest = c // (2 * len(QA) * wm), c % (2 * len(QA) * wm)
    ij, p6 = rest // len(QA), rest % len(QA)
    i, j = ij >> 1, ij & 1
    if half:
        return (f"acc[{i}][{j}] = __builtin_amdgcn_mfma_f32_32x32x16_f16(SXH(a[{s2}][{i}][{QA[p6]}]), SXH(b[{s2}][{j}][{QB[p6]}]), "
                f"acc[{i}][{j}], 0, 0, 0);")
    return f"acc[{i}][{j}] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[{s2}][{i}][{QA[p6]}], b[{s2}][{j}][{QB[p6]}], acc[{i}][{j}], 0, 0, 0);"


def by_weight(its, n):
    """the statements of n slots: every item, in order, goes to the slot in which the midpoint of its weight falls"""
    slots, total, done = [[] for _ in range(n)], sum(w for w, _ in its), 0
    for w, L in its:
        slots[(2 * done + w) * n // (2 * total)] += L
        done += w
    return slots


def by_count(its, n):
    return [[s for _, L in its[c * len(its) // n:(c + 1) * len(its) // n] for s in L] for c in range(n)]


def body(wm, variant="", half=False):
    """the lines of one K-tile body"""
    S = 4 * len(pieces(half)[0]) * wm
    early, rest = items(wm, variant, half)
    if half:
        slots = by_weight(early, S // 2) + by_weight(rest, S // 2)
    else:
        slots = by_weight(rest, S) if variant else by_count(rest, S)
    out = []
    for c, L in enumerate(slots):
        if half and c == S // 2:
            out.append("__syncthreads();     // every wave holds the fragments of both k16 steps: the images may be overwritten")
        out += [f"// slot {c}", mfma(c, wm, half)] + L + ["__builtin_amdgcn_sched_barrier(0);"]
    return out


def ladder():
    """the lines of the generated file: one `if constexpr` branch per VARIANTS row, the body of either tile height inside"""
    out = []
    for (npc, dy, xf, xd), v in VARIANTS.items():
        out.append(f"{'} else ' if out else ''}if constexpr (NPC == {npc} && DY == {str(dy).lower()} && XF == {xf} && XD == {str(xd).lower()}) {{")
        for wm in (2, 1):
            out.append(f"{'if (WM == 2) {' if wm == 2 else '} else {'}     // body({wm}, \"{v}\", {npc == 2})")
            out += body(wm, v, npc == 2)
        out.append("}")
    return out + ["} else static_assert(NPC < 0, \"gemm_split_kernel: no K-tile body for this instantiation (gen_split_body.py VARIANTS)\");"]


def main(path):
    text = "\n".join(ladder()) + "\n"
    with open(path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main(sys.argv[1])

"""CPU proof of tests/helpers/rowops_ref.py before tests/test_gpu_rowops.py trusts it: the reference equals the one-line fp64 operation,
the `exact` family is exact in fp32 in any order, an fp32 emulation of every kernel in its own order (the stand-in for the device) sits
inside the bound and not far below it, every reference mutant leaves the bound at every shape the GPU file runs, the scale-array port
equals the decode the GEMM tests use, and the GPU parametrisation reaches every norm cell and every pair of the gemm_f32 lists."""
import itertools

import pytest
import torch

from helpers import rowops_ref as rr

F64, F32 = torch.float64, torch.float32
FLOOR = 0.01                   # the emulation must come above 1 % of the bound somewhere on `normal`: the bound is not blind


def _close(y, want):
    assert (y - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item())


# ---- norms ----
NORM_CASES = rr.norm_cases()


def test_norm_cases_reach_every_cell_and_every_family():
    seen = {}
    for rows, H, group, ln, dt, fams in NORM_CASES:
        assert not rr.norm_refused(rows, H, group, 1, False)
        for form in rr.norm_forms(H, group):
            seen.setdefault(rr.norm_cell(ln, dt, form, H, group), set()).update(fams)
    assert set(seen) == set(rr.NORM_CELLS)
    assert all(s == set(rr.NORM_FAMILIES) for s in seen.values()), seen
    assert rr.norm_kernel(520, 1) == "rows8" and rr.norm_kernel(132, 1) == "rows4" and rr.norm_kernel(64, 4) == "rows4"


@pytest.mark.parametrize("case", NORM_CASES, ids=lambda c: f"{c[0]}x{c[1]}g{c[2]}-{'ln' if c[3] else 'rms'}-{c[4]}")
def test_norm_reference_emulation_and_bound(case):
    rows, H, group, ln, dt, fams = case
    for fam in fams + (("normal",) if "normal" not in fams else ()):
        for form in rr.norm_forms(H, group):
            P = rr.make_norm(ln, dt, form, rows, H, group, fam)
            y, e, E = rr.norm_reference(P)
            if form == "lo8" or dt == "bf16":
                _close(y, rr.norm_naive(P))
            r = rr.ratio((rr.norm_emulate(P) - y).abs(), E)
            assert r <= 1.0, (case, fam, form, r)
            if fam == "normal":
                assert r >= FLOOR, (case, form, r)
    if ln and dt == "f16":                                       # zero row: LayerNorm gives b, RMSNorm 0, the one-byte form scale 127 and zero bytes
        for lnz in (True, False):
            P = rr.make_norm(lnz, dt, "lo8" if group == 1 and H % 128 == 0 else "split", rows, H, group, "zero_row")
            y32, _ = rr.norm_values(P, F32)
            z = y32.reshape(rows, H)[rows // 2]
            assert torch.equal(z, P.b if lnz else torch.zeros(H))
            if P.form == "lo8" and not lnz:
                parts = rr.norm_encode(y32, dt, "lo8")
                assert bool((parts[1][rows // 2] == 0).all()) and bool((parts[2][rows // 2] == 127).all())


@pytest.mark.parametrize("case", [c for c in NORM_CASES if c[4] == "f16"], ids=lambda c: f"{c[0]}x{c[1]}g{c[2]}-{'ln' if c[3] else 'rms'}")
def test_norm_mutants_are_caught(case):
    rows, H, group, ln, dt, _ = case
    forms = rr.norm_forms(H, group)
    for mutant in rr.NORM_MUTANTS:
        form = forms[-1] if mutant.startswith("scale_") else "split"
        base = rr.make_norm(ln, dt, form, rows, H, group, "normal")
        if not rr.norm_applicable(mutant, base):
            continue
        worst = 0.0
        for fam in rr.NORM_FAMILIES:
            P = rr.make_norm(ln, dt, form, rows, H, group, fam)
            _, _, E = rr.norm_reference(P)
            ym, _, _ = rr.norm_reference(P, mutant)
            worst = max(worst, rr.ratio((rr.norm_emulate(P) - ym).abs(), E))
            if worst > 1.0:
                break
        assert worst > 1.0, (case, mutant, worst)


def test_norm_refusals_as_data():
    assert rr.norm_refused(4, 6, 1, 0, False) and rr.norm_refused(4, 4100, 1, 0, False) and rr.norm_refused(5, 64, 4, 0, False)
    assert rr.norm_refused(4, 128, 1, 0, True) and rr.norm_refused(4, 128, 2, 1, True) and rr.norm_refused(4, 192, 1, 1, True)
    assert not rr.norm_refused(4, 128, 1, 1, True) and not rr.norm_refused(8, 64, 4, 1, False)


# ---- the scale array of the one-byte form ----
@pytest.mark.parametrize("M,K", [(1, 128), (257, 640), (513, 512), (700, 384), (300, 1280)])
def test_lo8_scale_at_port_equals_the_decode_of_the_gemm_tests(M, K):
    nb = rr.lo8_scale_bytes(M, K)
    idx = rr.lo8_scale_index(M, K)
    assert idx.unique().numel() == idx.numel() and int(idx.max()) < nb
    for r, kb in [(0, 0), (M - 1, K // 128 - 1), (M // 2, (K // 128) // 2), (min(M - 1, 255), 0), (min(M - 1, 256), K // 128 - 1)]:
        assert int(idx[r, kb]) == rr.lo8_scale_at(r, kb, M)
    E = torch.randint(0, 255, (M, K // 128), dtype=torch.uint8, generator=torch.Generator().manual_seed(M + K))
    scales = torch.full((nb,), 255, dtype=torch.uint8)
    scales[idx.flatten()] = E.flatten()
    assert torch.equal(rr.lo8_scales_decode(scales, M, K), E)
    if M > 256:
        assert not torch.equal(rr.lo8_scale_index(M, K, tile_ignored=True), idx)


# ---- gemm_f32 ----
GEMM_CASES = rr.gemm_cases()


def test_gemm_cases_are_pairwise_and_hold_the_lists():
    lists = [rr.GEMM_M, rr.GEMM_N, rr.GEMM_K, (1, 0), (0, 1), (0, 1), rr.GEMM_ALPHA]
    for i, j in itertools.combinations(range(7), 2):
        assert {(c[i], c[j]) for c in GEMM_CASES} == set(itertools.product(lists[i], lists[j])), (i, j)
    assert len(GEMM_CASES) <= 80 and {"exact", "normal", "outlier"} == {c[7] for c in GEMM_CASES}
    assert any(c[7] == "exact" and c[2] == 300 for c in GEMM_CASES) and any(c[7] == "exact" and c[2] == 17 for c in GEMM_CASES)


@pytest.mark.parametrize("case", GEMM_CASES, ids=lambda c: "-".join(f"{v:.3g}" if isinstance(v, float) else str(v) for v in c))
def test_gemm_f32_reference_emulation_bound_and_mutants(case):
    for fam in dict.fromkeys((case[7], "normal", "exact")):
        if fam == "exact" and case[6] == rr.GEMM_ALPHA[2]:
            continue
        P = rr.make_gemm(*case[:7], fam)
        y, E = rr.gemm_run(P, F64)
        _close(y, rr.gemm_naive(P))
        emu, _ = rr.gemm_run(P, F32)
        if fam == "exact":                                      # exact in three orders: k ascending, k descending, torch's blocked matmul
            B = (P.Bmem if P.b_nt else P.Bmem.t())
            rev = torch.zeros(P.M, P.N)
            for k in reversed(range(P.K)):
                rev = rev + P.A[:, k, None] * B[None, :, k]
            for got in (emu, P.alpha * rev, P.alpha * (P.A @ B.t())):
                assert torch.equal(got.double(), y), case
        r = rr.ratio((emu.double() - y).abs(), E)
        assert r <= 1.0, (case, fam, r)
        if fam == "normal" and P.K >= 15:
            assert r >= FLOOR, (case, r)
        if P.K == 0:
            assert bool((y == 0).all()) and bool((emu == 0).all())
    for mutant in rr.GEMM_MUTANTS:
        worst, tried = 0.0, False
        for fam in ("normal", "outlier", "exact"):
            P = rr.make_gemm(*case[:7], fam)
            if not rr.gemm_applicable(mutant, P):
                continue
            tried = True
            _, E = rr.gemm_run(P, F64)
            ym, _ = rr.gemm_run(P, F64, mutant)
            worst = max(worst, rr.ratio((rr.gemm_run(P, F32)[0].double() - ym).abs(), E))
            if worst > 1.0:
                break
        assert not tried or worst > 1.0, (case, mutant, worst)


# ---- the reward tail ----
TAIL_CASES = [(op, kw) for op, cases in rr.tail_cases().items() for kw in cases]


def _tail_id(c):
    return c[0] + "-" + "-".join(f"{k}{v if not isinstance(v, list) else '_'.join(map(str, v))}" for k, v in c[1].items())


FLOOR_SEEN = {}


def _is_copy(P):
    """Cases whose result is an input value unchanged: nothing rounds."""
    return (P.op == "gather_norm" and P.w is None) or (P.op == "ca_pool" and P.o is None and P.u is None and P.S == 1) or \
        (P.op in ("ca_softmax", "ca_softmax_pad") and P.Vmax == 1)


def test_tail_cases_hold_the_issue_edges():
    cs = rr.tail_cases()
    sc = cs["ca_scores"]
    assert {c["Vmax"] for c in sc} == set(rr.TAIL_VMAX) and {c["B"] for c in sc} == set(rr.TAIL_B) and {c["vs"] for c in sc} == {0, 1}
    assert {c["D"] for c in sc} == set(rr.TAIL_D)
    for op in ("ca_scores", "ca_context"):
        vbs = [(v, c["Vmax"]) for c in cs[op] for v in c["vb"]]
        assert any(v == 0 for v, _ in vbs) and any(v == m for v, m in vbs) and {v % 4 for v, _ in vbs} == {0, 1, 2, 3}
    assert {c["D"] for c in cs["ca_pool"]} >= {64, 4096} and {c["S"] for c in cs["ca_pool"]} >= {1, 300}
    assert {(c["has_o"], c["has_u"]) for c in cs["ca_pool"]} == set(itertools.product((True, False), repeat=2))
    assert {c["pad"] for c in cs["ca_pool"]} == {"left", "right"}
    assert {c["d"] for c in cs["reward_head"]} == {1, 2, 10} and {c["attn_o"] for c in cs["reward_head"]} == {True, False}
    assert {(c["use_last_pos"], c["weight"]) for c in cs["gather_norm"]} == set(itertools.product((0, 1), (True, False)))
    pad = cs["ca_softmax_pad"]
    assert any(c["vb"] == c["Vmax"] for c in pad) and any(c["vb"] < c["Vmax"] for c in pad) and any(c["ld"] > c["vb"] for c in pad)
    assert all(c["ld"] % 4 == 0 and c["ld"] >= c["vb"] for c in pad)
    assert sum(len(v) for v in cs.values()) <= 120


@pytest.mark.parametrize("case", TAIL_CASES, ids=_tail_id)
def test_tail_reference_emulation_bound_and_mutants(case):
    op, kw = case
    caught = {m: None for m in rr.TAIL_MUTANTS[op]}
    for fam in rr.TAIL_FAMILIES[op]:
        if fam == "all_low" and kw["Vmax"] == kw["vb"]:
            continue
        P = rr.make_tail(op, fam, **kw)
        y, E = rr.tail_run(P, F64)
        _close(y, rr.tail_naive(P))
        emu = rr.tail_run(P, F32)[0].double()
        r = rr.ratio((emu - y).abs(), E)
        assert r <= 1.0, (case, fam, r)
        if fam == "normal":
            FLOOR_SEEN[op] = max(FLOOR_SEEN.get(op, 0.0), r)
            if y.numel() >= 64 and not _is_copy(P):             # (the largest of a handful of roundings is no statistic)
                assert r >= FLOOR, (case, r)
        if op == "gather_norm" and P.w is None:
            assert torch.equal(emu, y)                          # a copy
        if fam == "exact":                                      # exact in three orders: the kernel's, the reverse, torch's own
            if op == "rowvec_linear":
                others = [P.x.flip(1) @ P.W.flip(1).t(), P.x @ P.W.t()]
            elif op == "ca_scores":
                others = [torch.stack([torch.cat([P.scale * (P.ev[int(P.voff[b * P.vs]):int(P.voff[b * P.vs + 1])].flip(1) @ P.kq[b].flip(0)),
                                                  torch.zeros(P.Vmax - P.vb[b])]) for b in range(P.B)])]
                others.append(rr.tail_naive(P).float())
            else:
                others = [torch.stack([P.pr[b, :P.vb[b]].flip(0) @ P.ev[int(P.voff[b * P.vs]):int(P.voff[b * P.vs + 1])].flip(0) for b in range(P.B)])]
                others.append(rr.tail_naive(P).float())
            for got in [emu] + others:
                assert torch.equal(got.double(), y), (case, "exact")
        if op == "ca_scores":
            for b in range(P.B):
                assert bool((emu[b, P.vb[b]:] == 0).all())
        if op == "ca_pool":
            assert bool((emu[P.mask.sum(dim=1) == 0] == 0).all())
        for m in caught:
            if caught[m] is not True and rr.tail_applicable(m, P):
                ym, _ = rr.tail_run(P, F64, m)
                caught[m] = rr.ratio((emu - ym).abs(), E) > 1.0
    assert all(v is not False for v in caught.values()), (case, caught)


def test_zz_every_tail_kernel_comes_above_the_floor_on_normal():
    assert set(FLOOR_SEEN) == set(rr.TAIL_MUTANTS), "run after the parametrised tail test"
    assert all(v >= FLOOR for v in FLOOR_SEEN.values()), FLOOR_SEEN


def test_every_tail_mutant_is_applicable_somewhere():
    for op, cases in rr.tail_cases().items():
        for m in rr.TAIL_MUTANTS[op]:
            assert any(rr.tail_applicable(m, rr.make_tail(op, "normal", **kw)) for kw in cases), (op, m)

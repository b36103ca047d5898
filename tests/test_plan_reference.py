"""CPU proof of tests/helpers/plan_ref.py before tests/test_gpu_plan.py trusts it: the qwen plan reference equals transformers' own
get_rope_index (recorded in golden/plan_qwen_rope_index.json) on valid and masked entries alike, and so do synth.qwen_rope_index and
qwen_synth_batch's positions; the su-RoPE tables the reference model itself produced (golden/plan_su_rope_tables.json) lie inside the table
bound of the fp64 reference, with the same factor set on both sides of the boundary; the token plan reference equals the torch lines the
kernel cites; every reference mutant is rejected by at least one case of the GPU case lists (integers by inequality, tables by
err > bound, rope_split by bits) while every un-mutated fp32 emulation passes; and the reference model's rotate_half form, interleaved,
is the pair form."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import plan_ref as pr
from llava_reward_amd import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F64 = torch.float32, torch.float64


def _golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def _bits(rows):
    return torch.tensor(rows, dtype=torch.int32).view(F32)


# ---- qwen plan ----
QWEN = _golden("plan_qwen_rope_index.json")
_QCFG = synth.qwen_tiny_config(vocab_size=151680, image_token_id=pr.Q_IMAGE, pad_token_id=pr.Q_PAD)


def test_qwen_fixture_holds_the_case_list():
    assert set(QWEN["cases"]) == set(pr.qwen_cases()) and QWEN["image_token"] == pr.Q_IMAGE and QWEN["spatial_merge_size"] == pr.Q_MERGE
    for name in pr.qwen_cases():
        P, rec = pr.make_qwen(name), QWEN["cases"][name]
        assert P.ids.tolist() == rec["ids"] and P.mask.tolist() == rec["mask"] and [list(g) for g in P.grid_thw] == rec["grid_thw"]
        assert P.B == 3 and P.S in pr.QWEN_S and bool(P.mask.any(axis=1).all())
    assert {pr.make_qwen(n).S for n in pr.qwen_cases()} == set(pr.QWEN_S)


@pytest.mark.parametrize("name", list(pr.qwen_cases()))
def test_qwen_reference_equals_get_rope_index_and_synth(name):
    P = pr.make_qwen(name)
    pos3, img_row, rstat = pr.qwen_run(P)
    want = np.array(QWEN["cases"][name]["pos3"], np.int64)
    assert np.array_equal(pos3, want), name                       # valid and masked entries alike
    assert bool((want[:, P.mask == 0] == 0).all())
    if P.grid_thw:
        assert np.array_equal(pos3, synth.qwen_rope_index(P.ids, P.mask, P.grid_thw, _QCFG))
    # the image rows: slot j of image k in order of appearance, through slot2row; text and masked tokens -1
    slots = img_row[(P.ids == pr.Q_IMAGE) & (P.mask != 0)]
    assert slots.tolist() == P.slot2row.tolist() and int((img_row >= 0).sum()) == P.n_slots
    assert rstat[:, 0].sum() == len(P.grid_thw) and rstat[:, 1].tolist() == (P.ids == pr.Q_CA).sum(axis=1).tolist()


def test_qwen_reference_equals_synth_batch_positions():
    for seed, caps, grids in ((21, [6, 3], [(16, 16), (16, 16)]), (22, [5, 9, 2], [(8, 20), (12, 16), (6, 4)])):
        cfg = synth.qwen_tiny_config()
        b = synth.qwen_synth_batch(cfg, seed, caps, grids, with_pixels=False)
        thw = [tuple(int(v) for v in g) for g in b["image_grid_thw"]]
        n = sum(h * w // 4 for _, h, w in thw)
        pos3, _, _ = pr.qwen_plan_ref(b["input_ids"], b["attention_mask"], thw, cfg.vision.merge, cfg.image_token_id, -1, np.arange(n))
        assert np.array_equal(pos3, synth.qwen_rope_index(b["input_ids"], b["attention_mask"], thw, cfg))


def test_qwen_case_list_holds_what_the_kernel_can_get_wrong():
    """Runs that begin at lanes 0 and 63, cross one and two chunk boundaries, hold a masked hole, gh > gw and gw > gh, a row behind a row
    with several images, ca tokens among masked tokens."""
    starts, crossings, holes, shapes, after_multi, ca_masked = set(), set(), 0, set(), False, False
    for name in pr.qwen_cases():
        P = pr.make_qwen(name)
        _, _, rstat = pr.qwen_run(P)
        for b in range(P.B):
            kept = [t for t in range(P.S) if P.mask[b, t] != 0]
            runs = []
            for i, t in enumerate(kept):
                if P.ids[b, t] == pr.Q_IMAGE:
                    if i and P.ids[b, kept[i - 1]] == pr.Q_IMAGE:
                        runs[-1][1] = t
                    else:
                        runs.append([t, t])
            for s0, e0 in runs:
                starts.add(s0 % 64)
                crossings.add(e0 // 64 - s0 // 64)
                holes += int((P.mask[b, s0:e0 + 1] == 0).any())
            after_multi |= b > 0 and rstat[b - 1, 0] > 1 and rstat[b, 0] > 0
            ca_masked |= bool(((P.ids[b] == pr.Q_CA) & (P.mask[b] == 0)).any())
        shapes |= {np.sign(h - w) for _, h, w in P.grid_thw}
    assert {0, 63} <= starts and {1, 2} <= crossings and holes >= 2 and shapes == {-1, 0, 1} and after_multi and ca_masked


def _caught(mutants, cases, make, run, differ):
    """Every mutant differs from the reference on at least one case; returns mutant -> the cases that catch it."""
    by = {m: [] for m in mutants}
    for c in cases:
        P = make(c)
        ref = run(P)
        for m in mutants:
            if differ(ref, run(P, m)):
                by[m].append(c)
    missed = [m for m, v in by.items() if not v]
    assert not missed, f"no case of the GPU list catches {missed}: extend the list"
    return by


def _ints_differ(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


def test_qwen_mutants_are_caught():
    _caught(pr.QWEN_PLAN_MUTANTS, list(pr.qwen_cases()), pr.make_qwen, pr.qwen_run, _ints_differ)


def test_qwen_clamped_cases_stay_in_range():
    for which in ("runs", "long"):
        P = pr.make_qwen_clamped(which)
        pos3, img_row, rstat = pr.qwen_run(P)
        assert int(img_row.max()) < P.n_slots and int(img_row.min()) >= -1 and int(pos3.min()) >= 0
        assert rstat[:, 0].sum() > len(P.grid_thw) or int(((P.ids == pr.Q_IMAGE) & (P.mask != 0)).sum()) > P.n_slots


# ---- token plan ----
TP_CASES = pr.token_plan_cases()


def _torch_token_plan(P):
    """The lines the kernel cites, in torch: rw_model:344-345, :420/439, modeling_phi3_v.py:228."""
    ids = torch.from_numpy(P.ids)
    mask = torch.ones_like(ids) if P.mask is None else torch.from_numpy(P.mask)
    pos = mask.long().cumsum(-1) - 1
    pos.masked_fill_(mask == 0, 1)
    last = mask.size(1) - 1 - mask.long().fliplr().argmax(dim=1)
    slots = (ids == P.image_token_id) if P.image_token_id >= 0 else ((ids < 0) & (ids > -int(1e9)))
    return pos, last, slots


@pytest.mark.parametrize("case", TP_CASES, ids=lambda c: f"S{c[0]}-{c[1]}-{'_'.join(c[2])}")
def test_token_plan_reference_equals_the_cited_lines(case):
    P = pr.make_token_plan(case)
    pos, img_row, tstat = pr.token_plan_run(P)
    tpos, tlast, tslots = _torch_token_plan(P)
    if P.pos_arange:
        assert np.array_equal(pos, np.tile(np.arange(P.S), (P.B, 1)))
    else:
        valid = np.ones_like(P.ids, bool) if P.mask is None else P.mask != 0
        assert np.array_equal(pos, np.where(valid, tpos.numpy() + P.pos_base, 1))
    assert tstat[:, 0].tolist() == tlast.tolist()
    for b in range(P.B):
        v0 = int(P.voff[b * P.vs])
        cap = int(P.voff[b * P.vs + 1]) - v0
        at = torch.nonzero(tslots[b]).flatten().tolist()          # row-major order of index_put
        base = P.img_base or 0
        want = np.full(P.S, -1)
        for r, s in enumerate(at):
            if base + r < cap:
                want[s] = v0 + base + r
        assert np.array_equal(img_row[b], want)
        assert tstat[b, 2] == base + len(at) and tstat[b, 3] == (P.S if P.mask is None else int(P.mask[b].sum()))
        assert tstat[b, 1] == (0 if P.mask is None else (int(np.nonzero(P.mask[b])[0][0]) if P.mask[b].any() else P.S))


def test_token_plan_case_list_holds_the_issue_s_cases():
    assert {c[0] for c in TP_CASES} == set(pr.TP_S)
    for S in pr.TP_S:
        kinds = {k for c in TP_CASES if c[0] == S for k in c[2]}
        assert {m for m in pr.TP_MASKS if pr._tp_applicable(m, S)} <= kinds, (S, kinds)
        assert {c[1] for c in TP_CASES if c[0] == S} >= ({"phi", "prefixed"} | ({"llava"} if S > 1 else set()))
    rel, straddle = set(), set()
    for c in TP_CASES:
        P = pr.make_token_plan(c)
        _, img_row, tstat = pr.token_plan_run(P)
        for b in range(P.B):
            cap = int(P.voff[b * P.vs + 1]) - int(P.voff[b * P.vs])
            rel.add((c[1] == "prefixed", int(np.sign(int(tstat[b, 2]) - cap))))
            sl = (P.ids[b] == P.image_token_id) if P.image_token_id >= 0 else ((P.ids[b] < 0) & (P.ids[b] > pr.NOT_A_SLOT))
            for edge in (64, 256):
                if P.S > edge and sl[edge - 1] and sl[edge]:
                    straddle.add(edge)
        assert bool((P.ids <= pr.NOT_A_SLOT).any()) or P.S < 3
    assert rel == {(p, r) for p in (False, True) for r in (-1, 0, 1)} and straddle == {64, 256}


def test_token_plan_mutants_are_caught():
    by = _caught(pr.TOKEN_PLAN_MUTANTS, TP_CASES, pr.make_token_plan, pr.token_plan_run, _ints_differ)
    assert all(c[0] > 256 for c in by["carry_dropped_at_256"]) and all(c[0] > 64 for c in by["wave_prefix_off_by_one"])


def test_slot_check_reference():
    tstat = np.array([[0, 0, 5, 1], [0, 0, 4, 1], [0, 0, 0, 1]])
    r = np.arange(6, dtype=np.float32).reshape(3, 2)
    out = pr.slot_check_ref(tstat, np.array([0, 5, 10, 10]), r, 1)
    assert np.array_equal(out[0], r[0]) and np.isnan(out[1]).all() and np.array_equal(out[2], r[2])
    out = pr.slot_check_ref(tstat, np.array([3, 7, 99, 99]), r, 0)
    assert np.isnan(out[0]).all() and np.array_equal(out[1], r[1]) and np.isnan(out[2]).all()


# ---- embedding ----
def test_embed_reference_and_mutants():
    for rows, D, with_ev in pr.embed_cases():
        P = pr.make_embed(rows, D, with_ev)
        y = pr.embed_ref(P.ids, P.img_row, P.wte, P.ev, P.vocab)
        ids = torch.from_numpy(P.ids).clamp_min(0).clamp_max(P.vocab - 1)
        want = P.wte[:P.vocab].float()[ids]
        if with_ev:
            sel = torch.from_numpy(P.img_row) >= 0
            want[sel] = P.ev[torch.from_numpy(P.img_row)[sel]]
        assert torch.equal(y, want)
    by = _caught(pr.EMBED_MUTANTS, pr.embed_cases(), lambda c: pr.make_embed(*c),
                 lambda P, m=None: pr.embed_ref(P.ids, P.img_row, P.wte, P.ev, P.vocab, m), lambda a, b: not torch.equal(a, b))
    assert by
    ids = {int(v) for c in pr.embed_cases() for v in pr.make_embed(*c).ids}
    assert {0, 36, 37, 2 ** 40} <= ids and min(ids) < 0


# ---- tables ----
SU = _golden("plan_su_rope_tables.json")


def test_recorded_su_tables_lie_within_the_bound_and_pick_the_same_factors():
    """The reference model alone stays inside the bound: its fp32 cos / sin against fp64 of the fp32 angle, times its scaling factor."""
    hd, orig = SU["head_dim"], SU["original_max_position_embeddings"]
    assert (hd, orig, SU["positions"]) == (96, pr.ROPE_ORIG_MAX, [0, 1, 7, 8, 4095, 131071]) and set(SU["tables"]) == {"8", "9"}
    inv_s, inv_l = pr.rope_inv(hd, SU["rope_theta"])
    assert tuple(SU["short_factor"]) == synth.default_rope_factors(hd, 1.0, 0.004) and tuple(SU["long_factor"]) == synth.default_rope_factors(hd, 1.0, 0.8)
    scaling = pr.f32(SU["scaling_factor"])
    assert scaling == pr.su_scaling(SU["max_position_embeddings"], orig) and scaling > 1.0
    pos = np.array(SU["positions"])
    worst = 0.0
    for seq, t in SU["tables"].items():
        inv = _bits(t["inv_freq_bits"])
        want_long = pr.use_long(int(seq), orig)
        assert want_long == (int(seq) > orig) and torch.equal(inv, inv_l if want_long else inv_s) and not torch.equal(inv_s, inv_l)
        y, E = pr.rope_table_ref(pos, int(seq), inv_s, inv_l, scaling, orig)
        got = torch.stack([_bits(t["cos_bits"]), _bits(t["sin_bits"])], dim=-1)
        r = pr.table_ratio(got, y, E)
        assert r <= 1.0, (seq, r)
        worst = max(worst, r)
        # the other factor set, or the boundary one token early, leaves the bound
        assert pr.table_ratio(got, *pr.rope_table_ref(pos, int(seq), inv_s, inv_l, scaling, orig, mutant="switch_at_ge")) > 1.0 or int(seq) != orig
        assert pr.table_ratio(got, *pr.rope_table_ref(pos, int(seq), inv_l, inv_s, scaling, orig)) > 1.0
    print(f"recorded su-RoPE tables: max err / bound {worst:.3g}")


def _table_cases():
    return [("rope_table", c) for c in pr.rope_table_cases()] + [("mrope_table", c) for c in pr.mrope_cases()] + [("vit_rope_table", c) for c in pr.vit_cases()]


def _table_make(kc):
    kind, c = kc
    P = {"rope_table": pr.make_rope_table, "mrope_table": pr.make_mrope, "vit_rope_table": pr.make_vit}[kind](*c)
    P.kind = kind
    return P


def _table_run(P, mutant=None):
    if P.kind == "rope_table":
        return pr.rope_table_run(P, mutant)
    if P.kind == "mrope_table":
        return pr.mrope_table_ref(P.pos3, P.inv, P.s0, P.s1, mutant)
    return pr.vit_rope_table_ref(P.hw, P.inv, P.quarter, P.half_pad, mutant)


def _table_emulate(P):
    """The kernel's fp32 arithmetic on the CPU: the fp32 angle, torch's fp32 cos / sin, one fp32 product with scaling."""
    if P.kind == "rope_table":
        inv = P.inv_l if (P.rot if P.rot > 0 else P.S) > P.orig_max else P.inv_s
        return pr.table_emulate(torch.from_numpy(P.pos).to(F32)[:, None] * inv[None, :], P.scaling)
    if P.kind == "mrope_table":
        cs = torch.zeros(P.rows, P.half, 2)
        for k in range(P.half):
            st = 0 if k < P.s0 else (1 if k < P.s0 + P.s1 else 2)
            cs[:, k] = pr.table_emulate(torch.from_numpy(P.pos3[st]).to(F32) * P.inv[k], 1.0)
        return cs
    cs = torch.zeros(P.rows, P.half_pad, 2)
    cs[:, :, 0] = 1.0
    for k in range(2 * P.quarter):
        cs[:, k] = pr.table_emulate(torch.from_numpy(P.hw[:, 0 if k < P.quarter else 1].copy()).to(F32) * P.inv[k % P.quarter], 1.0)
    return cs


def test_table_emulations_pass_and_mutants_are_caught():
    cases = _table_cases()
    for kc in cases:
        P = _table_make(kc)
        y, E = _table_run(P)
        r = pr.table_ratio(_table_emulate(P), y, E)
        assert r <= 1.0, (kc, r)
    for kind, mutants in pr.TABLE_MUTANTS.items():
        _caught(mutants, [kc for kc in cases if kc[0] == kind], _table_make,
                lambda P, m=None: _table_run(P, m)[0] if m else _table_run(P), lambda ref, mut: pr.table_ratio(mut, *ref) > 1.0)


def test_table_case_lists_hold_the_issue_s_cases():
    rc = pr.rope_table_cases()
    assert {c[0] for c in rc} == {48, 64} and any(c[1] * c[2] == 12 for c in rc)
    assert {(c[2], c[3] - c[2] if c[3] else -1) for c in rc if c[2] in (8, 9)} == {(S, d) for S in (8, 9) for d in (-1, 0, 1)}
    assert {c[4] for c in rc} == {"su", "one"}
    for c in rc:
        assert set(pr.make_rope_table(*c).pos.tolist()) == set(pr.ROPE_POS)
    assert [(c[0], c[1], c[2]) for c in pr.mrope_cases()] == [(64, 16, 24), (64, 0, 0), (8, 2, 3)]
    assert [(c[0], c[1]) for c in pr.vit_cases()] == [(20, 48), (8, 16)] and pr.make_vit(*pr.vit_cases()[0]).hw.max(axis=0).tolist() == [200, 3]


# ---- rope_split ----
RS_CASES = pr.rope_split_cases()


def _np_rope_split(P, dt, prec):
    """An independent fp32 evaluation, element by element in numpy: the stand-in for the device."""
    q, cs = P.qkv.numpy(), P.cs.numpy()
    out = q.copy()
    for col in range(0, P.rope_cols, 2):
        i = (col % P.hd) // 2
        x, y, c, s = q[:, col], q[:, col + 1], cs[:, i, 0], cs[:, i, 1]
        out[:, col] = (x * c).astype(np.float32) - (y * s).astype(np.float32)
        out[:, col + 1] = (y * c).astype(np.float32) + (x * s).astype(np.float32)
    return pr._encode(torch.from_numpy(out), dt, prec)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int16), b.view(torch.int16))


def test_rope_split_emulation_equals_the_reference_and_mutants_are_caught():
    cells = [(c, dt, prec) for c in RS_CASES for dt in ("bf16", "f16") for prec in (0, 1)]
    for c, dt, prec in cells:
        P = pr.make_rope_split(*c)
        assert _same_bits(_np_rope_split(P, dt, prec), pr.rope_split_ref(P.qkv, P.cs, P.rope_cols, P.v_cols, P.hd, dt, prec)), (c, dt, prec)
    _caught(pr.ROPE_SPLIT_MUTANTS, cells, lambda c: (pr.make_rope_split(*c[0]), c[1], c[2]),
            lambda a, m=None: pr.rope_split_ref(a[0].qkv, a[0].cs, a[0].rope_cols, a[0].v_cols, a[0].hd, a[1], a[2], m), lambda a, b: not _same_bits(a, b))
    assert {c[1] for c in RS_CASES} == {8, 64, 96, 128} and {c[2] for c in RS_CASES} >= {768, 2304} and {c[3] for c in RS_CASES} == {0, 4, 1028}
    assert {c[0] for c in RS_CASES} == {1, 3} and {c[4] for c in RS_CASES} == set(pr.RS_FAMILIES)
    for c in RS_CASES:
        if c[4] == "exact":                                       # products and sums exact: the fp64 evaluation has the same fp32 values
            P = pr.make_rope_split(*c)
            q = P.qkv[:, :P.rope_cols].double().view(P.rows, -1, P.hd // 2, 2)
            cc, ss = P.cs[:, None, :, 0].double(), P.cs[:, None, :, 1].double()
            want = torch.stack([q[..., 0] * cc - q[..., 1] * ss, q[..., 1] * cc + q[..., 0] * ss], dim=-1).reshape(P.rows, -1)
            got = pr.rope_split_ref(P.qkv, P.cs, P.rope_cols, P.v_cols, P.hd, "f16", 1)
            n = P.rope_cols + P.v_cols
            assert torch.equal((got[:, :n].double() + got[:, n:].double())[:, :P.rope_cols], want)


def test_rotate_half_form_interleaved_is_the_pair_form():
    """q cos + rotate_half(q) sin on the reference's layout (dims i and i + hd/2), interleaved, equals the pair form on the interleaved
    input bit for bit in fp32: the pair-interleave convention itself."""
    g = torch.Generator().manual_seed(5)
    for hd, heads, rows in ((8, 1, 3), (96, 4, 5), (128, 2, 2)):
        q = torch.randn(rows, heads, hd, generator=g)
        ang = torch.rand(rows, hd // 2, generator=g) * 6.3
        cos, sin = torch.cos(ang) * 1.19, torch.sin(ang) * 1.19
        want = pr.interleave(pr.rotate_half_ref(q, cos, sin)).reshape(rows, heads * hd)
        qi = pr.interleave(q).reshape(rows, heads * hd)
        cs = torch.stack([cos, sin], dim=-1)
        for dt in ("bf16", "f16"):
            got = pr.rope_split_ref(qi, cs, heads * hd, 0, hd, dt, 1)
            assert _same_bits(got, pr._encode(want, dt, 1))
        # and the scalar products of two rotated heads do not see the permutation
        k = torch.randn(rows, heads, hd, generator=g)
        a, b = pr.rotate_half_ref(q.double(), cos.double(), sin.double()), pr.rotate_half_ref(k.double(), cos.double(), sin.double())
        assert torch.allclose((a * b).sum(-1), (pr.interleave(a) * pr.interleave(b)).sum(-1), rtol=1e-12, atol=1e-12)


def test_rope_split_refusals():
    assert pr.rope_split_refused(12, 24, 0) and pr.rope_split_refused(8, 20, 0) and pr.rope_split_refused(8, 16, 6) and not pr.rope_split_refused(8, 16, 4)

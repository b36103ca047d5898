"""CPU proof of tests/helpers/vision_ref.py before tests/test_gpu_vision.py trusts it, and of the host plans that run in the product.
The references equal the real programs as recorded in golden/vision_*.{npz,json} (the reference tree's hd_feature_transform,
transformers' pack_image_features / unpad_image / select_best_resolution and get_vision_window_index / get_vision_position_ids) and
synth's restatements; the two host-only entries of the library (lr_vision_sample_plan, lr_qwen_vision_plan: the C++ the forwards run)
equal the references on the fixture cases and on the sweeps, and lr_llava_image_geometry's select_best_resolution -- a second C++ copy
-- picks the same resolution as the plan on every swept size; every reference mutant is rejected by at least one case of the GPU case
lists (copies by bits, clip_embed by err > bound) while the un-mutated fp32 emulation passes."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from helpers import vision_ref as vr
from llava_reward_amd import _lib, synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32, F64 = torch.float32, torch.float64
HD = np.load(os.path.join(GOLDEN, "vision_hd_transform.npz"))
QW = np.load(os.path.join(GOLDEN, "vision_qwen_window.npz"))
with open(os.path.join(GOLDEN, "vision_llava_pack.json")) as _f:
    LV = json.load(_f)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()                                            # the host entries need no device


# ---- Phi-3-V HD transform ----
def _hd_index_features(ncrops, g, H):
    """clipx [ncrops, g g + 1, H]: patch token t of crop c holds (c g g + t) H + channel, CLS holds -99."""
    v = (torch.arange(ncrops * g * g, dtype=F32)[:, None] * H + torch.arange(H)).reshape(ncrops, g * g, H)
    return torch.cat([torch.full((ncrops, 1, H), -99.0), v], dim=1)


def _hd_source_map(grids, ncrop_per_image, g=24, H=2):
    smp, rows = [], 0
    for i, (a, b) in enumerate(grids):
        smp.append((a, b, i * ncrop_per_image, rows))
        rows += vr.hd_plan_ref(a, b, 1, g)[3]
    out = vr.hd_gather_values(_hd_index_features(len(grids) * ncrop_per_image, g, H), smp, g, torch.full((4 * H,), -1.0), torch.full((4 * H,), -2.0))
    assert out.shape == (rows, 4 * H)
    blocks = out.reshape(rows, 4, H)
    sep = blocks[:, :, 0] < 0
    assert bool((blocks[:, :, 1] == blocks[:, :, 0] + (~sep).float()).all()), "a block is not one token's channels"
    m = torch.where(sep, blocks[:, :, 0], torch.div(blocks[:, :, 0], H, rounding_mode="floor")).long().numpy()
    for (_, _, crop0, voff), nxt in zip(smp, [s[3] for s in smp[1:]] + [rows]):      # the fixture counts crops per image
        part = m[voff:nxt]
        part[part >= 0] -= crop0 * g * g
    return m


@pytest.mark.parametrize("grid", vr.HD_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_hd_reference_equals_the_reference_tree(grid):
    want = np.cumsum(HD[f"g{grid[0]}x{grid[1]}"], axis=0)
    assert want.shape[0] == vr.hd_plan_ref(*grid, 1, 24)[3] == synth.num_img_tokens(grid[0] * 336, grid[1] * 336)
    assert np.array_equal(_hd_source_map([grid], grid[0] * grid[1] + 1), want)


def test_hd_reference_equals_the_reference_tree_on_a_batch():
    assert np.array_equal(_hd_source_map(list(vr.HD_BATCH), int(HD["batch_ncrop"])), np.cumsum(HD["batch"], axis=0))


def test_hd_plan_entry(lib):
    for g in (2, 4, 6, 24):
        crop = 14 * g
        for a in range(1, 6):
            for b in range(1, 6):
                rc, smp, nc, nr = vr.lib_sample_plan(lib, vr.LR_BACKBONE_PHI3V, crop, g, None, a * crop, b * crop)
                assert rc == 0 and (smp, nc, nr) == ([a, b, 0, 0], *vr.hd_plan_ref(a * crop, b * crop, crop, g)[2:])
    for h, w in ((0, 336), (336, -336), (337, 336), (336, 100)):
        assert vr.lib_sample_plan(lib, vr.LR_BACKBONE_PHI3V, 336, 24, None, h, w)[0] != 0
    assert vr.lib_sample_plan(lib, vr.LR_BACKBONE_PHI3V, 336, 23, None, 336, 336)[0] != 0       # odd CLIP grid
    assert vr.lib_sample_plan(lib, 2, 336, 24, None, 336, 336)[0] != 0                          # no such plan for Qwen


# ---- LLaVA anyres ----
def _llava_rows(geom, g):
    """Source row (crop g g + token, -1 = newline) of every packed row, from the reference on index-valued features."""
    gh, gw = geom[:2]
    proj = torch.arange((1 + gh * gw) * g * g, dtype=F32).reshape(1 + gh * gw, g * g, 1)
    return vr.llava_pack_ref(proj, [tuple(geom[:6]) + (0, 0)], g, torch.tensor([-1.0]))[:, 0].long().tolist()


def _check_llava_record(rec, plan, g):
    gh, gw, r0, r1, c0, c1, ncr, V = plan
    assert r0 <= r1 and c0 <= c1 and V == g * g + (r1 - r0) * (c1 - c0 + 1) and ncr == 1 + gh * gw
    if "raised" in rec:                                           # the real program gave up: only the invariants above are pinned
        return
    assert (gh, gw) == (rec["gh"], rec["gw"]) and [r1 - r0, c1 - c0] == rec["kept"] and V == rec["rows"], rec
    if "r0" in rec:
        assert (r0, r1, c0, c1) == (rec["r0"], rec["r1"], rec["c0"], rec["c1"]), rec
    rows = _llava_rows(plan, g)
    assert vr.digest(rows) == rec["digest"]
    if "source" in rec:
        assert rows == rec["source"]


@pytest.mark.parametrize("key", ["g4", "g24", "g24_reordered"])
def test_llava_reference_and_plan_entry_equal_transformers(lib, key):
    crop, g = LV[key]["crop"], LV[key]["g"]
    re = key.endswith("reordered")
    pins = vr.pinpoints_reordered(crop) if re else vr.pinpoints(crop)
    sizes = vr.REORDERED_SIZES(crop) if re else vr.llava_sizes(crop)
    assert [(r["h"], r["w"]) for r in LV[key]["cases"]] == sizes and LV["pinpoint_grids"] == [list(p) for p in vr.LLAVA_PINPOINT_GRIDS]
    empty = 0
    for rec in LV[key]["cases"]:
        plan = vr.llava_plan_ref(rec["h"], rec["w"], pins, crop, g)
        _check_llava_record(rec, plan, g)
        rc, smp, nc, nr = vr.lib_sample_plan(lib, vr.LR_BACKBONE_LLAVA_NEXT, crop, g, pins, rec["h"], rec["w"])
        assert rc == 0 and tuple(smp[:6]) + (nc, nr) == plan and smp[6:] == [0, 0], (rec["h"], rec["w"], smp, plan)
        if not re:
            assert plan[:6] + plan[7:] == synth.llava_geometry(rec["h"], rec["w"], tuple(pins), crop, g)
        empty += 0 in rec["kept"]
    if not re:
        assert empty >= 2 and {(1, 2000), (2000, 1)} <= set(sizes)      # the strips whose unpad leaves no rows / no columns


def test_llava_case_list_holds_what_the_plan_can_get_wrong():
    """Both unpad branches, pad = 0, every pinpoint, a switch between every pair of resolutions that meet, a size at which truncation and
    int(round(x, 7)) part, the aspect boundary itself."""
    crop, g, pins = 336, 24, vr.pinpoints(336)
    plans = {s: vr.llava_plan_ref(*s, pins, crop, g) for s in vr.llava_sizes(crop)}
    assert {p[:2] for p in plans.values()} == set(vr.LLAVA_PINPOINT_GRIDS)
    assert any(p[2] > 0 for p in plans.values()) and any(p[4] > 0 for p in plans.values())
    assert sum(1 for p in plans.values() if p[2] == 0 and p[4] == 0 and p[3] == p[0] * g and p[5] == p[1] * g) >= 5
    assert any(w * p[0] == h * p[1] for (h, w), p in plans.items()), "no size sits on the aspect boundary"
    assert any(p[4] < g < p[5] for p in plans.values() if p[1] > 1), "no kept column range straddles two crops"


def test_llava_plan_sweep_against_synth_the_library_and_the_image_geometry(lib):
    """Every swept (h, w): reference == synth.llava_geometry == lr_vision_sample_plan, and lr_llava_image_geometry (preprocess.hip's own
    select_best_resolution) picks the plan's resolution."""
    crop, g, pins = 336, 24, vr.pinpoints(336)
    assert tuple(pins) == synth.LLAVA_PINPOINTS
    pin = (C.c_int32 * 10)(*[v for p in pins for v in p])
    smp, nc, nr, geo = (C.c_int32 * 8)(), C.c_int32(), C.c_int32(), (C.c_int32 * 5)()
    sweep = vr.llava_sweep()
    assert len(sweep) == 44946
    for h, w in sweep:
        plan = vr.llava_plan_ref(h, w, pins, crop, g)
        assert plan[:6] + plan[7:] == synth.llava_geometry(h, w)
        assert lib.lr_vision_sample_plan(vr.LR_BACKBONE_LLAVA_NEXT, crop, g, pin, 5, h, w, smp, C.byref(nc), C.byref(nr)) == 0
        assert tuple(smp[:6]) + (nc.value, nr.value) == plan, (h, w, list(smp), plan)
        assert lib.lr_llava_image_geometry(h, w, pin, 5, geo) == 0
        assert (geo[0], geo[1], geo[4]) == (plan[0] * crop, plan[1] * crop, plan[6]), (h, w, list(geo), plan)


def test_llava_plan_entry_refusals(lib):
    pins = vr.pinpoints(336)
    L = vr.LR_BACKBONE_LLAVA_NEXT
    assert vr.lib_sample_plan(lib, L, 336, 24, pins, 0, 5)[0] != 0 and vr.lib_sample_plan(lib, L, 336, 24, pins, 5, -1)[0] != 0
    assert vr.lib_sample_plan(lib, L, 336, 24, None, 5, 5)[0] != 0 and vr.lib_sample_plan(lib, L, 336, 24, pins * 2, 5, 5)[0] != 0
    assert vr.lib_sample_plan(lib, L, 336, 24, [(336, 100)], 5, 5)[0] != 0 and vr.lib_sample_plan(lib, L, 0, 24, pins, 5, 5)[0] != 0
    assert vr.lib_sample_plan(lib, L, 336, 0, pins, 5, 5)[0] != 0


# ---- Qwen window plan ----
def _qwen_fixture(name):
    names = json.loads(str(QW["names"]))
    i = names.index(name)
    off = QW["lengths"][:i].sum(axis=0)
    n = QW["lengths"][i]
    return (QW["window_index"][off[0]:off[0] + n[0]].astype(np.int64), QW["cu_window_seqlens"][off[1]:off[1] + n[1]].astype(np.int64),
            QW["position_ids"][off[2]:off[2] + n[2]].astype(np.int64))


def _check_plan_shape(p, grids, merge=vr.QWEN_MERGE):
    """What any plan must satisfy, whatever the window order: src a permutation, slot2row its inverse on units, items covering the rows."""
    unit = merge * merge
    N = sum(a * b for a, b in grids)
    assert p.counts[0] == N and sorted(p.src.tolist()) == list(range(N))
    assert np.array_equal(p.src[p.slot2row * unit] // unit, np.arange(N // unit))
    for items in (p.items_win, p.items_full):
        covered = []
        for row0, n, q, z in items.tolist():
            assert z == 0 and 0 <= q * 128 < n
            if q == 0:
                covered += list(range(row0, row0 + n))
        assert covered == list(range(N))
    assert p.counts[3] == max(int(p.items_win[:, 1].max()), int(p.items_full[:, 1].max()))


@pytest.mark.parametrize("name", list(vr.qwen_fixture_cases()))
def test_qwen_reference_and_plan_entry_equal_transformers(lib, name):
    grids = vr.qwen_fixture_cases()[name]
    assert json.loads(str(QW["names"])) == list(vr.qwen_fixture_cases())
    wi, cu, pos = _qwen_fixture(name)
    p = vr.qwen_window_plan_ref(grids, vr.QWEN_MERGE, vr.QWEN_WS)
    unit = vr.QWEN_MERGE ** 2
    assert np.array_equal(p.src.reshape(-1, unit), wi[:, None] * unit + np.arange(unit)), "window order"
    assert np.array_equal(p.cu, cu), "cu_window_seqlens"
    assert np.array_equal(p.hw, pos[p.src]), "row r carries the position of processor patch src[r]"
    _check_plan_shape(p, grids)
    rc, q = vr.lib_qwen_plan(lib, grids)
    assert rc == 0
    for a, b, what in zip(vr.plan_outputs(p), vr.plan_outputs(q), ("src", "hw", "slot2row", "items_win", "items_full", "imgs", "counts")):
        assert np.array_equal(a, b), (name, what)


def test_qwen_fixture_holds_even_and_uneven_grids():
    sides = {a for a in vr.QWEN_SIDES}
    assert {s % vr.QWEN_WS == 0 for s in sides} == {True, False} and min(sides) < vr.QWEN_WS < max(sides) and 2 * vr.QWEN_WS in sides
    assert sorted(len(g) for n, g in vr.qwen_fixture_cases().items() if "x" not in n) == [2, 2, 3]
    _, cu, _ = _qwen_fixture("4x8")                               # divides evenly: the extra windows stay empty and leave no boundary
    assert cu.tolist() == [0, 64, 128]


def test_qwen_plan_sweep_against_synth_and_the_library(lib):
    vc = synth.QwenVisionConfig()
    assert (vc.merge, vc.window_merged, vc.window, vc.patch) == (vr.QWEN_MERGE, vr.QWEN_WS, vr.QWEN_WINDOW, vr.QWEN_PATCH)
    sweep = vr.qwen_sweep()
    assert len(sweep) == 338
    unit = vc.merge_unit
    for grids in sweep:
        p = vr.qwen_window_plan_ref(grids, vr.QWEN_MERGE, vr.QWEN_WS)
        thw = [(1, a, b) for a, b in grids]
        idx, cu = synth.qwen_window_index(thw, vc)
        assert np.array_equal(p.src[::unit] // unit, idx) and np.array_equal(p.cu, cu)
        assert np.array_equal(p.hw, synth.qwen_patch_positions(thw, vc)[p.src])
        assert np.array_equal(p.items_win[p.items_win[:, 2] == 0][:, 0], cu[:-1])
        rc, q = vr.lib_qwen_plan(lib, grids)
        assert rc == 0
        for a, b in zip(vr.plan_outputs(p), vr.plan_outputs(q)):
            assert np.array_equal(a, b), grids


def test_qwen_plan_entry_other_geometries_and_refusals(lib):
    """merge 1 and 3, a window of 3 merged tokens, an image above 128 rows per window item (two 128-query tiles); then what it refuses."""
    for grids, merge, window, patch in (([(5, 7)], 1, 42, 14), ([(9, 12), (3, 3)], 3, 126, 14), ([(64, 64)], 2, 1792, 14), ([(40, 36)], 2, 112, 14)):
        p = vr.qwen_window_plan_ref(grids, merge, window // merge // patch)
        rc, q = vr.lib_qwen_plan(lib, grids, merge, window, patch)
        assert rc == 0
        _check_plan_shape(p, grids, merge)
        for a, b in zip(vr.plan_outputs(p), vr.plan_outputs(q)):
            assert np.array_equal(a, b), grids
    assert int(vr.qwen_window_plan_ref([(64, 64)], 2, 64).items_win[:, 2].max()) >= 1
    for grids, kw in (([(3, 4)], {}), ([(0, 4)], {}), ([(4, 4)], {"merge": 0}), ([(4, 4)], {"patch": 0}), ([(4, 4)], {"window": 14}), ([(128, 66)], {}),
                      ([(4, 4)], {"capacity": 15}), ([(4, 4)], {"merge": 12, "window": 1000})):
        assert vr.lib_qwen_plan(lib, grids, **kw)[0] != 0, (grids, kw)
    thw = (C.c_int64 * 3)(2, 4, 4)                                # a video grid
    buf = (C.c_int32 * 64)()
    assert lib.lr_qwen_vision_plan(thw, 1, 2, 112, 14, 16, buf, buf, buf, buf, buf, buf, buf) != 0


# ---- mutants ----
def _caught(op, cases, differ):
    by = {m: [] for m in vr.MUTANTS[op]}
    for c in cases:
        for m in vr.MUTANTS[op]:
            if differ(c, m):
                by[m].append(c)
    missed = [m for m, v in by.items() if not v and m not in vr.EQUIVALENT_MUTANTS.get(op, ())]
    assert not missed, f"no case of the GPU list catches {missed}: extend the list"
    return by


def _bits_differ(make, ref):
    def differ(case, m):
        P = make(case)
        return any(not torch.equal(ref(P, dt, prec).view(torch.int16), ref(P, dt, prec, m).view(torch.int16)) for dt in vr.DTS for prec in (0, 1))
    return differ


def test_copy_mutants_are_caught():
    _caught("im2col", vr.im2col_cases(), _bits_differ(vr.make_im2col, vr.im2col_ref))
    _caught("hd_gather", vr.hd_gather_cases(), _bits_differ(vr.make_hd_gather, vr.hd_gather_ref))
    _caught("clip_tokens", vr.clip_tokens_cases(), _bits_differ(vr.make_clip_tokens, vr.clip_tokens_ref))
    _caught("qwen_patch_gather", vr.qwen_gather_cases(), _bits_differ(vr.make_qwen_gather, vr.qwen_gather_ref))

    def pack_differ(case, m):
        P = vr.make_llava_pack(case)
        return not torch.equal(vr.llava_pack_ref(P.proj, P.samples, P.g, P.newline), vr.llava_pack_ref(P.proj, P.samples, P.g, P.newline, m))
    _caught("llava_pack", vr.llava_pack_cases(), pack_differ)


def test_plan_mutants_are_caught():
    def qdiffer(name, m):
        g = vr.qwen_fixture_cases()[name]
        a, b = vr.qwen_window_plan_ref(g, vr.QWEN_MERGE, vr.QWEN_WS), vr.qwen_window_plan_ref(g, vr.QWEN_MERGE, vr.QWEN_WS, m)
        return any(not np.array_equal(x, y) for x, y in zip(vr.plan_outputs(a), vr.plan_outputs(b)))
    by = _caught("qwen_window_plan", list(vr.qwen_fixture_cases()) + ["big"], lambda n, m: qdiffer(n, m) if n != "big" else any(
        not np.array_equal(x, y) for x, y in zip(vr.plan_outputs(vr.qwen_window_plan_ref([(40, 36)], 2, 4)), vr.plan_outputs(vr.qwen_window_plan_ref([(40, 36)], 2, 4, m)))))
    assert vr.EQUIVALENT_MUTANTS["qwen_window_plan"] == ("no_empty_extra_window",) and not by["no_empty_extra_window"]

    def ldiffer(case, m):
        crop, g, re, (h, w) = case
        pins = vr.pinpoints_reordered(crop) if re else vr.pinpoints(crop)
        return vr.llava_plan_ref(h, w, pins, crop, g) != vr.llava_plan_ref(h, w, pins, crop, g, m)
    cases = [(c, g, False, s) for c, g in ((336, 24), (56, 4)) for s in vr.llava_sizes(c)] + [(336, 24, True, s) for s in vr.REORDERED_SIZES(336)]
    by = _caught("llava_plan", cases, ldiffer)
    assert vr.EQUIVALENT_MUTANTS["llava_plan"] == ("aspect_test_ge",) and not by["aspect_test_ge"]
    assert not any(ldiffer((336, 24, False, s), "aspect_test_ge") for s in vr.llava_sweep()[::7]), "aspect_test_ge is no longer equivalent: list a case"


def test_hd_case_list_has_ragged_totals():
    """Every (g, H) meets a total row count that is no multiple of 4 (the kernel serves 4 rows per block), gaps in front of the crops, and
    all five grids."""
    for g in vr.HD_G:
        assert any(vr.make_hd_gather((g, 4, B)).rows % 4 for B in (1, 2, 3)), g
    assert {gr for b in vr.HD_BATCHES.values() for gr in b} == {(1, 1), (1, 2), (2, 1), (2, 3), (3, 1)}
    P = vr.make_hd_gather((6, 4, 3))
    assert not bool(P.used.all()) and P.samples[0][2] > 0


def test_llava_pack_cases_cover_the_geometries():
    for g in vr.LLAVA_G:
        geoms = [tuple(s[:6]) for B in (1, 2, 3) for s in vr.make_llava_pack((g, 4, B)).samples.tolist()]
        assert any(r0 > 0 for _, _, r0, _, _, _ in geoms) and any(c0 > 0 and c1 > c0 for _, _, _, _, c0, c1 in geoms)
        assert any((gh * g, gw * g) == (r1 - r0, c1 - c0) for gh, gw, r0, r1, c0, c1 in geoms), "pad = 0"
        assert any(gw == 1 for _, gw, *_ in geoms) and any(r0 == r1 for _, _, r0, r1, _, _ in geoms), "one-column grid, zero-row unpad"
        assert any(gw > 1 and c0 >= g and c1 > c0 for _, gw, _, _, c0, c1 in geoms) and any(gw > 1 and c0 < g < c1 for _, gw, _, _, c0, c1 in geoms)
        assert any(vr.make_llava_pack((g, 4, B)).rows % 4 for B in (1, 2, 3))


# ---- clip_embed ----
@pytest.mark.parametrize("case", vr.clip_embed_cases(), ids=lambda c: f"H{c[0]}-T{c[1]}")
def test_clip_embed_reference_bound_and_mutants(case):
    P = vr.make_clip_embed(case)
    y, e = vr.clip_embed_run(P, F64)
    assert float((y - vr.clip_embed_naive(P)).abs().max()) < 1e-11, "the ordered reference is not the module"
    emu, _ = vr.clip_embed_run(P, F32)
    r = vr.ratio((emu.double() - y).abs(), e)
    print(f"[clip_embed H{P.H} T{P.T}] fp32 emulation max err / bound {r:.3g}")
    assert r <= 1.0
    assert bool((e > 0).all()) and float((e / (1 + y.abs())).max()) < 1e-5, "the bound is too loose to mean anything"
    for m in vr.MUTANTS["clip_embed"]:
        ym, _ = vr.clip_embed_run(P, F64, m)
        assert vr.ratio((ym - y).abs(), e) > 1.0, (case, m)

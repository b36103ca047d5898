"""Every attention kernel form (csrc/attention.hip launch_one: 22 (head_dim, causal, split, waves, ping-pong, ragged) cells x 2 operand
types) against the fp64 reference and per-element rounding bound of tests/helpers/attention_ref.py, at the sequence-length, mask, GQA,
ragged-segment and layout edges.  Every launch also checks that nothing outside the output rows and columns was written (canary rows
after the last sequence and gap columns, inside the allocation)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import attention_ref as ar
from llava_reward_amd import _lib as L
from llava_reward_amd import synth

pytestmark = pytest.mark.gpu

DT = {"bf16": (L.LR_DT_BF16, torch.bfloat16), "f16": (L.LR_DT_F16, torch.float16)}
GUARD = 3                      # canary rows after the last sequence
SENTINEL = 0x5A5A              # canary bits (finite in both operand types)
POISON = 3.0e4                 # gap columns of the operand rows: a kernel that reads them is far off


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return L.load()


def P(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def _ru8(x):
    return (x + 7) // 8 * 8


def _mask(B, S, spans):
    m = torch.ones(B, S, dtype=torch.int64)
    for b, sp in enumerate(spans):
        for a, e in sp:
            m[b, a:min(e, S)] = 0
    return m


def run(lib, dt, hd, causal, S, *, split=False, lazy=0.0, B=1, H=2, group=1, spans=None, segments=None, family="normal",
        layout=False, pingpong=1, seed=0, refuse=False):
    """One launch of the op for this form; returns max(err / bound).  segments: ragged mode (cu_seqlens, B = 1, S = total rows)."""
    code, tdt = DT[dt]
    prev = os.environ.get("LR_ATT_PINGPONG")
    os.environ["LR_ATT_PINGPONG"] = str(pingpong)         # read by launch_one per launch
    try:
        Hkv = H // group
        scale = 80 ** -0.5 if segments is not None else hd ** -0.5
        mask = _mask(B, S, spans) if spans is not None else None
        rows = B * S
        q, k, v = ar.make_inputs(family, B, S, H, Hkv, hd, scale=scale, mask=mask, segments=segments, seed=seed)
        wq, wkv = H * hd, Hkv * hd
        xs = [q.reshape(rows, wq), k.reshape(rows, wkv), v.reshape(rows, wkv)]
        parts = [ar.split(x, tdt) if split else (x.to(tdt), None) for x in xs]
        if layout:                               # separate buffers, non-zero offsets, poisoned gap columns (ldq larger than used)
            m = max(wq, wkv)
            offs = (8, 16, 24)
            lo_off = _ru8(24 + m + 8)
            ld = _ru8((lo_off if split else 0) + 24 + m + 8)
            bufs = [torch.full((rows + GUARD, ld), POISON, dtype=tdt) for _ in range(3)]
        else:                                    # the engine's packed [q | k | v] (| residuals) rows
            W = wq + 2 * wkv
            offs = (0, wq, wq + wkv)
            lo_off = W
            ld = 2 * W if split else W
            bufs = [torch.full((rows + GUARD, ld), POISON, dtype=tdt)] * 3
        for buf, off, (hi, lo) in zip(bufs, offs, parts):
            buf[:rows, off:off + hi.shape[1]] = hi
            if split:
                buf[:rows, off + lo_off:off + lo_off + lo.shape[1]] = lo
        bufs = [b.cuda() for b in bufs] if layout else [bufs[0].cuda()] * 3
        gap = 8 if layout else 0
        o_split = wq + gap if split else 0
        ldo = (o_split + wq if split else wq) + gap
        O = torch.full((rows + GUARD, ldo), SENTINEL, dtype=torch.int16, device="cuda").view(tdt)
        dmask = mask.cuda() if mask is not None else None
        kmin = torch.tensor([ar.kmin_of(mask[b]) for b in range(B)], dtype=torch.int32, device="cuda") if mask is not None else None
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        Q, K, V = bufs
        if segments is not None:
            cu = np.array(segments, dtype=np.int32)
            cp = cu.ctypes.data_as(C.POINTER(C.c_int32))
            if split:
                rc = lib.lr_op_attention_segments_split(P(Q), P(K), P(V), P(O), cp, len(cu) - 1, ld, ldo, *offs, lo_off, o_split, H, hd,
                                                        scale, lazy, code, st)
            else:
                rc = lib.lr_op_attention_segments(P(Q), P(K), P(V), P(O), cp, len(cu) - 1, ld, ldo, *offs, H, hd, scale, code, st)
        elif split:
            rc = lib.lr_op_attention_split_ex(P(Q), P(K), P(V), P(O), P(dmask), P(kmin), ld, ldo, *offs, lo_off, o_split, B, S, H, hd,
                                              int(causal), group, scale, lazy, code, st)
        else:
            rc = lib.lr_op_attention(P(Q), P(K), P(V), P(O), P(dmask), P(kmin), ld, ldo, *offs, B, S, H, hd, int(causal), group,
                                     scale, code, st)
        torch.cuda.synchronize()
        bits = O.view(torch.int16)
        if refuse:
            assert rc != 0 and bool((bits == SENTINEL).all()), "a refused launch wrote O"
            return 0.0
        assert rc == 0, L.last_error() if hasattr(L, "last_error") else rc
        # canaries: guard rows and gap columns untouched
        assert bool((bits[rows:] == SENTINEL).all()), "write past the last sequence row"
        written = torch.zeros(ldo, dtype=torch.bool, device="cuda")
        written[:wq] = True
        if split:
            written[o_split:o_split + wq] = True
        assert bool((bits[:rows, ~written] == SENTINEL).all()), "write into the gap columns of O"
        got = O[:rows, :wq].double() + (O[:rows, o_split:o_split + wq].double() if split else 0)
        vals = [(hi.double() + lo.double()) if split else hi.double() for hi, lo in parts]
        lo3 = [lo.double().cuda() for _, lo in parts] if split else None
        shp = [(B, S, H, hd), (B, S, Hkv, hd), (B, S, Hkv, hd)]
        qd, kd, vd = (x.cuda().view(s) for x, s in zip(vals, shp))
        if split:
            lo3 = [x.view(s) for x, s in zip(lo3, shp)]
        ref, bnd = ar.reference(qd, kd, vd, scale=scale, causal=causal, mask=dmask, segments=segments, kv_group=group, dtype=dt,
                                split=split, lo=lo3, lazy_t=lazy, chunk=512)
        err = (got.view(B, S, H, hd) - ref).abs()
        r = ar.max_ratio(err, bnd)
        inst = ar.dispatch(hd, causal, split, S, pingpong=bool(pingpong), ragged=segments is not None)
        print(f"[attn {dt}{'x2' if split else ''} hd={hd} causal={causal} S={S} B={B} H={H} g={group} inst={inst} "
              f"ragged={segments is not None} {family} lazy={lazy}] max err/bound {r:.3g}  max err {err.max().item():.3g}")
        assert r <= 1.0, r
        return r
    finally:
        if prev is None:
            os.environ.pop("LR_ATT_PINGPONG", None)
        else:
            os.environ["LR_ATT_PINGPONG"] = prev


# ---- every dispatch cell, both operand types ----
def _cell_cases():
    cases = []
    fams = ar.FAMILIES
    n = 0
    for (hd, causal) in ar.FORMS:
        spans = [[(0, 37)], [(0, 0)]] if causal else [[(70, 90)], [(0, 0)]]
        for split, S, pp in ((False, 300, 1), (False, 1100, 1), (False, 1100, 0), (True, 128, 1), (True, 577 if hd == 64 else 300, 1),
                             (True, 1100, 1), (True, 1100, 0)):
            lazy = 8.0 if n % 2 else 0.0
            cases.append(dict(hd=hd, causal=causal, S=S, split=split, pingpong=pp, B=2, H=2, spans=spans, family=fams[n % 3],
                              layout=n % 3 == 1, lazy=lazy if split else 0.0))
            n += 1
    for hd in (64, 96):
        for split in (False, True):
            cases.append(dict(hd=hd, causal=False, S=600, split=split, B=1, H=2, segments=[0, 64, 64, 65, 192, 600],
                              family=fams[n % 3], layout=n % 2 == 0))
            n += 1
    return cases


CELL_CASES = _cell_cases()
CELLS_HIT = {(c["hd"], c["causal"]) + ar.dispatch(c["hd"], c["causal"], c["split"], c["S"], bool(c.get("pingpong", 1)),
                                                   "segments" in c) + ("segments" in c,) for c in CELL_CASES}
assert CELLS_HIT == ar.all_cells(), ar.all_cells() ^ CELLS_HIT          # the parametrisation reaches every cell, the ragged ones included


def test_parametrisation_hits_every_dispatch_cell():
    assert CELLS_HIT == ar.all_cells() and len({c[:5] for c in CELLS_HIT}) == 22      # x 2 operand types: 44 instantiations


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("i", range(len(CELL_CASES)),
                         ids=[f"{c['hd']}{'c' if c['causal'] else 'd'}-{'x2' if c['split'] else 'x1'}-S{c['S']}-pp{c.get('pingpong', 1)}"
                              f"{'-ragged' if 'segments' in c else ''}" for c in CELL_CASES])
def test_dispatch_cell(lib, dt, i):
    run(lib, dt, seed=i, **CELL_CASES[i])


# ---- sequence-length edges (decoder form: head_dim 96 causal), left padding and a long interior hole ----
EDGE_S = [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2642, 4095, 4096, 4097, 8192]


@pytest.mark.parametrize("S", EDGE_S)
def test_sequence_length_edges(lib, S):
    km = S // 3
    spans = [[(0, km)] + ([(S // 2, S // 2 + 600)] if S > 1300 else [])]
    fam = "ramp" if S % 2 else "poison"
    run(lib, "bf16" if S % 2 else "f16", 96, True, S, B=1, H=1, spans=spans, family=fam, seed=S)
    run(lib, "f16" if S % 2 else "bf16", 96, True, S, split=True, lazy=8.0 if S > 2000 else 0.0, B=1, H=1, spans=spans, family=fam, seed=S)


def test_sequence_longer_than_8192_is_refused(lib):
    for split in (False, True):
        run(lib, "bf16", 96, True, 8193, split=split, B=1, H=1, spans=[[(0, 5)]], refuse=True)


# ---- masks: left padding with kmin inside the last partial tile, right padding, holes over more than eight tiles, an all-padding row ----
MASK_SPANS = [[(0, 1090)], [(800, 1100)], [(100, 700), (900, 950)], [(0, 1100)], [(0, 37)]]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("form", [(96, True, False, 1100), (96, True, True, 1100), (64, True, False, 300), (128, True, True, 1100),
                                  (64, False, False, 1100), (96, False, True, 300)], ids=lambda f: f"{f[0]}{'c' if f[1] else 'd'}-x{2 if f[2] else 1}-S{f[3]}")
@pytest.mark.parametrize("family", ["poison", "ramp"])
def test_masks(lib, dt, form, family):
    hd, causal, split, S = form
    spans = [[(a, min(e, S)) for a, e in row if a < S] or [(0, 0)] for row in MASK_SPANS]
    spans[3] = [(0, S)]
    # (non-causal launches honour the key mask: the bitmask is built from it whatever the form; kmin only bounds causal launches)
    run(lib, dt, hd, causal, S, split=split, B=len(spans), H=1, spans=spans, family=family, seed=hd + S)


# ---- GQA groups, with batch x kv heads = 1 and 7 (mod 8) and above 8: the XCD-order grid decode ----
@pytest.mark.parametrize("group,B,KV", [(1, 3, 3), (2, 7, 1), (4, 1, 1), (7, 1, 1), (7, 7, 1), (7, 3, 3)])
def test_gqa_groups(lib, group, B, KV):
    spans = [[(0, 11 * b)] for b in range(B)]
    run(lib, "bf16" if group % 2 else "f16", 128, True, 300, B=B, H=group * KV, group=group, spans=spans, seed=group)
    run(lib, "f16" if group % 2 else "bf16", 128, True, 1100, split=True, B=B, H=group * KV, group=group, spans=spans, family="ramp",
        seed=group, layout=True)


# ---- ragged segments: images at max_pixels (5120 patches) and >= 4096 rows next to 0-, 1- and 127-row segments ----
@pytest.mark.parametrize("hd,split,dt", [(96, False, "bf16"), (96, True, "f16"), (64, False, "f16"), (64, True, "bf16")])
def test_ragged_long_segments(lib, hd, split, dt):
    lens = [5120, 0, 1, 127, 4100, 64]
    cu = [0] + np.cumsum(lens).tolist()
    run(lib, dt, hd, False, cu[-1], split=split, lazy=8.0 if split else 0.0, B=1, H=1, segments=cu, family="poison", layout=split)


# ---- engine level: the gathered last layer (one query tile per sequence, never shifted) against the full one (query tiles shifted
# towards the end of the sequence at S >= 1024), rows of 2642 and 1100 - 1330 tokens with left and right padding ----
def _mixed_padding(batch, right_rows):
    rp = synth.right_pad(batch)
    out = {k: v.copy() for k, v in batch.items()}
    for b in right_rows:
        out["input_ids"][b], out["attention_mask"][b] = rp["input_ids"][b], rp["attention_mask"][b]
    return out


@pytest.mark.parametrize("dtype", ["f16x2", "f16x2f8", "f16"])
@pytest.mark.parametrize("backbone", ["phi3v", "llava"])
def test_gathered_last_layer_equals_the_full_one_on_long_rows(dtype, backbone):
    from llava_reward_amd.model import RewardModel
    seed = 23
    targets = [2642, 1100, 1130] if backbone == "phi3v" else [2642, 1300, 1330]   # row lengths; rows 1 / 2: left / right padding
    if backbone == "phi3v":
        cfg = synth.tiny_config()
        V = synth.num_img_tokens(336, 336)
        batch = synth.synth_batch(cfg, seed, [t - V - 5 for t in targets], (1, 1))
        fwd = lambda m, tb: m.custom_forward(tb["input_ids"], tb["attention_mask"], tb["pixel_values"], tb["image_sizes"])[0]
        crops = 2
    else:
        cfg = synth.llava_tiny_config()
        V = synth.llava_geometry(336, 336, cfg.pinpoints)[6]
        crops = 5                                     # (the engine wants room for the largest anyres grid + 1)
        batch = synth.llava_synth_batch(cfg, seed, [t - V - 5 for t in targets], [(336, 336)] * 3, max_crops=crops)
        fwd = lambda m, tb: m.custom_forward(inputs_batch=tb)[0]
    batch = _mixed_padding(batch, [2])
    S = batch["input_ids"].shape[1]
    assert S == 2642 and int(batch["attention_mask"][1].sum()) == targets[1]
    assert batch["attention_mask"][1, 0] == 0 and batch["attention_mask"][2, -1] == 0
    m = RewardModel(cfg, synth_seed=seed, max_batch=3, max_seq=S, max_crops=crops, operand_dtype=dtype).to("cuda").eval()
    tb = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    m.keep_hidden_states = False
    gathered = fwd(m, tb).cpu()
    torch.cuda.synchronize()
    m.keep_hidden_states = True
    full = fwd(m, tb).cpu()
    torch.cuda.synchronize()
    print(f"[gathered vs full {backbone} {dtype}] rewards {gathered.flatten().tolist()}")
    assert torch.isfinite(gathered).all()
    assert torch.equal(gathered, full)

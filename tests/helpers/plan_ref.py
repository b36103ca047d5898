"""Plain references, bounds, reference mutants and case lists of the kernels that decide which position a token has, which image row
it reads and which rotation its q and k get (csrc/rowops.hip token_plan / slot_check / prefix_header / embed / rope_table / rope_split,
csrc/rowops_qwen.hip qwen_runs + qwen_plan / mrope_table / vit_rope_table / qwen_ca_vec), for tests/test_plan_reference.py (CPU) and
tests/test_gpu_plan.py (MI355X).  Built like helpers/rowops_ref.py.

The integer references are token-by-token Python loops over numpy arrays; they restate neither the kernels' ballot / prefix arithmetic nor
synth.qwen_rope_index (which the CPU file cross-checks against them and against transformers' own get_rope_index, recorded in
tests/golden/plan_qwen_rope_index.json).
  token plan: rw_model_general_preference.py:344-345 (cumsum(mask) - 1, pads -> 1), :420/439 (S - 1 - argmax(flip(mask))),
  modeling_phi3_v.py:228-249 (image slots = ids in (-1e9, 0), filled in row-major order); a slot beyond voff[b+1] - voff[b] keeps -1 (the
  kernel's documented contract).  tstat[b] = {last valid, first valid (S when none), slot rank after the row, valid tokens}.
  qwen plan: get_rope_index for still images: drop masked tokens, group the rest by type, text counts up from the running position, an
  image gets t = start, h / w = start + grid coordinates and advances the position by max(h, w) / merge.  Masked entries are 0.
Tables.  Reference angle = the fp32 product float32(pos) * inv[k] (the reference model's own single rounding, and the kernel's), then
fp64 cos / sin of that fp32 value, times scaling.  Bound per element: TRIG_ULP fp32 ulp of |cos| (|sin|), times scaling, plus one
rounding (u32 |value|) for the scaling product when scaling != 1.  No margin factor.  The (1, 0) pad pairs are exact.
rope_split.  rope_pair is compiled with contraction off, so the output equals BIT FOR BIT the operand rounding of the fp32 evaluation
x c - y s, y c + x s (two rounded products, one rounded sum); in split form lo = round(v - hi); v columns are rounded / split unchanged.
"""
import types

import numpy as np
import torch

from .gemm_ref import F16_MAX, TDT, U32

TRIG_ULP = 4                   # sinf / cosf: ulp charged.  Source: OpenCL's full-profile limit for sin / cos (4 ulp), which OCML implements;
                               # no HIP math API table was at hand (the rule rowops_ref applies to rsqrtf)
F32, F64 = torch.float32, torch.float64
NOT_A_SLOT = -10 ** 9          # modeling_phi3_v.py MAX_INPUT_ID: ids <= -1e9 are no image slots

TOKEN_PLAN_MUTANTS = ("carry_dropped_at_256", "wave_prefix_off_by_one", "pads_get_0", "slots_gated_by_mask", "pos_base_ignored",
                      "img_base_ignored", "voff_stride_ignored", "overflow_reads_on", "last_valid_is_count_minus_1", "all_pad_row_last_is_0",
                      "id_minus_1e9_is_a_slot")
QWEN_PLAN_MUTANTS = ("run_state_lost_at_64", "prev_type_ignores_mask_hole", "advance_is_h_not_max", "text_after_image_restarts_at_count",
                     "img_base_from_own_row_only", "j_div_gh_not_gw", "ca_count_gated_by_mask")
TABLE_MUTANTS = {"rope_table": ("long_by_valid_length", "switch_at_ge", "scaling_dropped", "sin_cos_swapped"),
                 "mrope_table": ("mrope_stream_boundary_off_by_one", "sin_cos_swapped"),
                 "vit_rope_table": ("vit_w_uses_inv_k", "pad_pair_zero", "sin_cos_swapped")}
ROPE_SPLIT_MUTANTS = ("fused_multiply_add", "table_index_per_column_not_per_head", "lo_of_unrounded_hi", "v_rotated")
EMBED_MUTANTS = ("clamp_to_vocab", "negative_id_wraps", "img_row_0_taken_as_text")


# ---------------------------------------------------------------------------------------------------------------------------------------
# token plan
# ---------------------------------------------------------------------------------------------------------------------------------------
def token_plan_ref(ids, mask, voff, image_token_id=-1, pos_arange=0, pos_base=0, img_base=0, voff_stride=1, mutant=None):
    """(pos [B, S], img_row [B, S], tstat [B, 4]) int64.  mask None: every token valid.  voff: the int array the kernel is given."""
    B, S = ids.shape
    pos = np.zeros((B, S), np.int64)
    img_row = np.full((B, S), -1, np.int64)
    tstat = np.zeros((B, 4), np.int64)
    vs = 1 if mutant == "voff_stride_ignored" else voff_stride
    for b in range(B):
        v0, cap = int(voff[b * vs]), int(voff[b * vs + 1]) - int(voff[b * vs])
        count, rank = 0, (0 if mutant == "img_base_ignored" else img_base)
        wave_counts = {}                                           # valid tokens per (chunk of 256, wave of 64): the off-by-one mutant only
        last, first = -1, S
        for s in range(S):
            if mutant == "carry_dropped_at_256" and s and s % 256 == 0:
                count, rank = 0, 0
            m = True if mask is None else bool(mask[b, s] != 0)
            t = int(ids[b, s])
            if image_token_id >= 0:
                slot = t == image_token_id
            else:
                slot = t < 0 and (t >= NOT_A_SLOT if mutant == "id_minus_1e9_is_a_slot" else t > NOT_A_SLOT)
            if mutant == "slots_gated_by_mask":
                slot = slot and m
            if pos_arange:
                pos[b, s] = s
            elif m:
                p = (0 if mutant == "pos_base_ignored" else pos_base) + count      # cumsum(mask) - 1 = valid tokens before this one
                if mutant == "wave_prefix_off_by_one" and (s % 256) // 64 >= 1:  # the prefix over the waves before this one misses the last of them
                    p -= wave_counts.get((s // 256, (s % 256) // 64 - 1), 0)
                pos[b, s] = p
            else:
                pos[b, s] = 0 if mutant == "pads_get_0" else 1
            if slot:
                if rank < cap or mutant == "overflow_reads_on":
                    img_row[b, s] = v0 + rank
                rank += 1
            if m:
                count += 1
                wave_counts[(s // 256, (s % 256) // 64)] = wave_counts.get((s // 256, (s % 256) // 64), 0) + 1
                last = s
                first = min(first, s)
        if last < 0:
            last = 0 if mutant == "all_pad_row_last_is_0" else S - 1
        elif mutant == "last_valid_is_count_minus_1":
            last = count - 1
        tstat[b] = (last, first, rank, count)
    return pos, img_row, tstat


TP_S = (1, 63, 64, 65, 255, 256, 257, 513, 600)
TP_MASKS = ("ones", "left", "right", "hole", "zero", "one@0", "one@last", "one@255", "one@256")
IMAGE_TOKEN = 32000            # LLaVA form: the one id that is an image slot


def _tp_mask(kind, S):
    m = np.zeros(S, np.int64)
    if kind == "ones":
        m[:] = 1
    elif kind == "left":
        m[min(S - 1, max(1, S // 3)):] = 1
    elif kind == "right":
        m[:max(1, S - max(1, S // 3))] = 1
    elif kind == "hole":
        m[:] = 1
        m[S // 2 - S // 8: S // 2 + S // 8 + (1 if S > 2 else 0)] = 0
        m[0] = 1
    elif kind == "zero":
        pass
    else:
        at = {"one@0": 0, "one@last": S - 1, "one@255": 255, "one@256": 256}[kind]
        m[at] = 1
    return m


def _tp_applicable(kind, S):
    return {"one@255": S > 255, "one@256": S > 256}.get(kind, True)


def token_plan_cases():
    """(S, form, mask kinds of the three rows, k): form 'phi' (negative ids are slots), 'llava' (id == IMAGE_TOKEN, pos = arange) or
    'prefixed' (mask == null, pos_base, *img_base, voff_stride 0).  Every mask kind meets every S at which it exists."""
    out, k = [], 0
    for S in TP_S:
        kinds = [m for m in TP_MASKS if _tp_applicable(m, S)]
        while len(kinds) % 3:
            kinds.append(kinds[len(kinds) % 5])
        for i in range(0, len(kinds), 3):
            out.append((S, "llava" if k % 3 == 2 else "phi", tuple(kinds[i:i + 3]), k))
            k += 1
        out.append((S, "prefixed", ("null", "null", "null"), k))
        k += 1
    return out


def make_token_plan(case):
    """The arguments of one launch.  Image-slot runs straddle tokens 63|64 and 255|256 (and sit in masked stretches); the slot count of the
    three rows is equal to, above and below voff[b+1] - voff[b] (rotating); ids <= -1e9 are decoys; voff starts above 0."""
    S, form, kinds, k = case
    B = 3
    g = np.random.default_rng(1000 + k)
    ids = g.integers(3, 1000, (B, S)).astype(np.int64)
    slot = IMAGE_TOKEN if form == "llava" else None
    nslots = []
    for b in range(B):
        at = set()
        for lo, hi in ((60 - b, 68 + b), (252 - b, 259 + b), (S // 3, S // 3 + max(1, S // 16)), (S - 1, S)):
            at |= set(range(max(lo, 0), min(hi, S)))
        if S == 1 and b == 1:
            at = set()
        for s in sorted(at):
            ids[b, s] = slot if slot is not None else -1 - int(g.integers(0, 50))
        nslots.append(len(at))
        for s in (S // 5, (2 * S) // 3 + 1):                        # decoys: no slots in either form
            if s < S and s not in at:
                ids[b, s] = NOT_A_SLOT if (s + b) % 2 else NOT_A_SLOT - 5
    P = types.SimpleNamespace(S=S, B=B, form=form, kinds=kinds, k=k, ids=ids, image_token_id=slot if slot is not None else -1,
                              pos_arange=1 if form == "llava" else 0, pos_base=0, img_base=None, vs=1)
    if form == "prefixed":
        P.mask = None
        P.pos_base, P.img_base, P.vs = 320 + k, 7 + k % 3, 0
        cap = P.img_base + (nslots[0], max(nslots[0] - 2, 0), nslots[0] + 3)[k % 3]        # one image for every row: equal / above / below for row 0
        P.voff = np.array([5, 5 + cap, 10 ** 6, 10 ** 6 + 1], np.int32)                 # entries behind 1: poison a kernel with stride 1 would read
    else:
        P.mask = np.stack([_tp_mask(kind, S) for kind in kinds])
        caps = [(n, max(n - 2, 0), n + 3)[(b + k) % 3] for b, n in enumerate(nslots)]
        P.voff = np.concatenate([[5], 5 + np.cumsum(caps)]).astype(np.int32)
    return P


def token_plan_run(P, mutant=None):
    return token_plan_ref(P.ids, P.mask, P.voff, P.image_token_id, P.pos_arange, P.pos_base, P.img_base or 0, P.vs, mutant)


def slot_check_ref(tstat, voff, rewards, vs):
    """rewards [B, d] with NaN rows where tstat[b][2] != voff[b*vs+1] - voff[b*vs]; the other rows keep their bits."""
    out = rewards.copy()
    for b in range(rewards.shape[0]):
        if int(tstat[b, 2]) != int(voff[b * vs + 1]) - int(voff[b * vs]):
            out[b] = np.nan
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------
# embedding
# ---------------------------------------------------------------------------------------------------------------------------------------
def embed_ref(ids, img_row, wte, ev, vocab, mutant=None):
    """x [rows, D] fp32: ev[img_row] where img_row >= 0, else wte[clamp(id, 0, vocab - 1)] (bf16 -> fp32).  wte may hold rows behind
    `vocab` (poison): only a mutant reads them."""
    rows = len(ids)
    out = torch.zeros(rows, wte.shape[1], dtype=F32)
    for r in range(rows):
        ir, t = int(img_row[r]), int(ids[r])
        if (ir > 0) if mutant == "img_row_0_taken_as_text" else (ir >= 0):
            out[r] = ev[ir]
            continue
        if t < 0:
            t = vocab + max(t, -vocab) if mutant == "negative_id_wraps" else 0
        t = min(t, vocab if mutant == "clamp_to_vocab" else vocab - 1)
        out[r] = wte[t].float()
    return out


EMBED_ROWS, EMBED_D = (1, 5, 9), (4, 256, 260, 3072)


def embed_cases():
    return [(rows, D, ev) for i, D in enumerate(EMBED_D) for j, rows in enumerate(EMBED_ROWS) for ev in ((True, False) if (i + j) % 2 == 0 else (True,))]


def make_embed(rows, D, with_ev, vocab=37, seed=0):
    g = torch.Generator().manual_seed(seed * 31 + rows * 7 + D)
    wte = torch.randn(vocab + 1, D, generator=g).bfloat16()
    wte[vocab] = 3.0e4                                            # the row behind the table
    nev = 6
    ev = torch.randn(nev, D, generator=g) if with_ev else None
    pool = [-3, 0, vocab - 1, vocab, 2 ** 40, 5, -2 ** 40, 11, vocab - 2]
    ids = np.array([pool[(r + rows) % len(pool)] for r in range(rows)], np.int64)
    img_row = np.full(rows, -1, np.int64)
    if with_ev:
        for r, v in zip(range(0, rows, 2), (0, nev - 1, 3, 0, nev - 1)):
            img_row[r] = v
    return types.SimpleNamespace(rows=rows, D=D, vocab=vocab, wte=wte, ev=ev, ids=ids, img_row=img_row)


# ---------------------------------------------------------------------------------------------------------------------------------------
# qwen plan
# ---------------------------------------------------------------------------------------------------------------------------------------
Q_IMAGE, Q_CA, Q_PAD, Q_MERGE = 151655, 151643, 151643, 2       # <|image_pad|>; the SkipCA token, which is also the pad token


def qwen_plan_ref(ids, mask, grid_thw, merge, image_token, ca_token, slot2row, mutant=None, clamp=False):
    """(pos3 [3, B, S], img_row [B, S], rstat [B, 4]) int64: get_rope_index for still images, the merger row of every image slot and the
    row statistics.  clamp: the kernel's documented clamping of a batch the host wrapper would refuse (a run beyond the last image reads
    the last image, a slot beyond its image reads the image's last slot, a slot index beyond the table its last entry)."""
    B, S = ids.shape
    pos3 = np.zeros((3, B, S), np.int64)
    img_row = np.full((B, S), -1, np.int64)
    rstat = np.zeros((B, 4), np.int64)
    first = np.concatenate([[0], np.cumsum([(h // merge) * (w // merge) for _, h, w in grid_thw])]).astype(np.int64) if len(grid_thw) else [0]
    k = 0
    for b in range(B):
        if mutant == "img_base_from_own_row_only":
            k = 0
        kept = [s for s in range(S) if mask[b, s] != 0]
        groups, prev_s = [], None
        for s in kept:
            typ = int(ids[b, s]) == image_token
            glued = groups and groups[-1][0] == typ
            if mutant == "prev_type_ignores_mask_hole" and typ and prev_s is not None and prev_s != s - 1:
                glued = False                                     # a masked token in front of an image slot starts a new run
            if glued:
                groups[-1][1].append(s)
            else:
                groups.append((typ, [s]))
            prev_s = s
        cur, seen, runs = 0, 0, 0
        for typ, members in groups:
            if not typ:
                if mutant == "text_after_image_restarts_at_count":
                    cur = seen
                for i, s in enumerate(members):
                    pos3[:, b, s] = cur + i
                cur += len(members)
            else:
                kk = min(k, len(grid_thw) - 1) if clamp or mutant else k      # (a mutant may ask for more images than there are)
                _, h, w = grid_thw[kk]
                gh, gw = h // merge, w // merge
                for j, s in enumerate(members):
                    if clamp:
                        j = min(j, gh * gw - 1)
                    jj = j
                    if mutant == "run_state_lost_at_64" and s // 64 != members[0] // 64:
                        jj = sum(1 for q in members if q >= s // 64 * 64 and q < s)        # the run's slot counter restarts with the chunk
                    pos3[0, b, s] = cur
                    pos3[1, b, s] = cur + (jj // gh if mutant == "j_div_gh_not_gw" else jj // gw)
                    pos3[2, b, s] = cur + (jj % gh if mutant == "j_div_gh_not_gw" else jj % gw)
                    slot = first[kk] + jj
                    img_row[b, s] = slot2row[min(slot, len(slot2row) - 1) if clamp or mutant else slot]
                cur += gh if mutant == "advance_is_h_not_max" else max(h, w) // merge
                k += 1
                runs += 1
            seen += len(members)
        nca = sum(1 for s in range(S) if int(ids[b, s]) == ca_token and (mutant != "ca_count_gated_by_mask" or mask[b, s] != 0))
        rstat[b] = (runs, nca, 0, 0)
    return pos3, img_row, rstat


def qwen_imgs(grid_thw, merge):
    """The kernel's image table [n][4] = {merged grid h, w, advance, first slot}."""
    out, first = [], 0
    for _, h, w in grid_thw:
        gh, gw = h // merge, w // merge
        out.append((gh, gw, max(h, w) // merge, first))
        first += gh * gw
    return np.array(out, np.int32).reshape(-1, 4)


def _qrow(S, segs, pad="left", k=0):
    """One row from segments: ('t', n) text, ('c', n) un-masked ca tokens, ('i', gh, gw) an image run, ('i', gh, gw, at, n, id) the same with
    n masked tokens `id` inserted in front of slot `at`; padded (masked pad tokens) to S.  Returns (ids, mask, grids in patches)."""
    ids, mask, grids = [], [], []
    for seg in segs:
        if seg[0] == "t":
            ids += [10 + (7 * (len(ids) + k)) % 900 for _ in range(seg[1])]
            mask += [1] * seg[1]
        elif seg[0] == "c":
            ids += [Q_CA] * seg[1]
            mask += [1] * seg[1]
        else:
            gh, gw = seg[1], seg[2]
            run, rm = [Q_IMAGE] * (gh * gw), [1] * (gh * gw)
            if len(seg) > 3:
                _, _, _, at, n, hid = seg
                run[at:at] = [hid] * n
                rm[at:at] = [0] * n
            ids += run
            mask += rm
            grids.append((1, gh * Q_MERGE, gw * Q_MERGE))
    n = S - len(ids)
    assert n >= 0, (S, len(ids))
    if pad == "left":
        ids, mask = [Q_PAD] * n + ids, [0] * n + mask
    else:
        ids, mask = ids + [Q_PAD] * n, mask + [0] * n
    return ids, mask, grids


QWEN_S = (1, 63, 64, 65, 130, 200)


def qwen_cases():
    """name -> (S, [three rows of _qrow arguments]): B = 3; no row is wholly masked (get_rope_index cannot place such a row)."""
    T, I = "t", "i"
    return {
        "s1": (1, [([(T, 1)], "left"), ([("c", 1)], "left"), ([(T, 1)], "right")]),
        # two images then text; a row after it (rstat prefix) with gh > gw, left padded; no image, right padded, ca tokens in the padding
        "s63": (63, [([(T, 3), (I, 4, 6), (T, 5), (I, 2, 3), (T, 25)], "left"), ([(T, 2), (I, 3, 2), (T, 40)], "left"), ([(T, 50)], "right")]),
        # runs beginning at lanes 0 and 63; three images separated by text, a masked hole inside the second; no image with un-masked ca tokens
        "s64": (64, [([(I, 5, 4), (T, 43), (I, 1, 1)], "left"),
                     ([(T, 1), (I, 2, 2), (T, 3), (I, 3, 4, 5, 2, Q_PAD), (T, 2), (I, 1, 3), (T, 30)], "left"), ([(T, 20), ("c", 3), (T, 30)], "right")]),
        # a run beginning at lane 63 that crosses into the next chunk; gw > gh followed by text; left and right padding
        "s65": (65, [([(T, 63), (I, 1, 2)], "left"), ([(T, 4), (I, 2, 7), (T, 30)], "left"), ([(T, 2), (I, 3, 1), (T, 9)], "right")]),
        # a hole of image-token ids inside a run that crosses token 64; a run that ends at lane 63 of the second chunk
        "s130": (130, [([(T, 50), (I, 5, 6, 12, 3, Q_IMAGE), (T, 40)], "left"), ([(T, 100), (I, 4, 7), (T, 2)], "left"),
                       ([(I, 2, 2), (T, 60), (I, 2, 2), (T, 1), (I, 6, 2, 6, 1, Q_PAD), (T, 30)], "right")]),
        # one image of 10 x 14 = 140 slots: the run crosses two chunk boundaries; then rows with two and three images
        "s200": (200, [([(T, 3), (I, 10, 14), (T, 57)], "left"), ([(T, 5), (I, 4, 4), (T, 30), (I, 7, 5, 20, 4, Q_PAD), (T, 60)], "left"),
                       ([(T, 1), (I, 2, 9), (T, 61), (I, 8, 3), ("c", 2), (T, 40), (I, 3, 3), (T, 20)], "right")]),
    }


def make_qwen(name):
    S, rows = qwen_cases()[name]
    ids, mask, grids = [], [], []
    for k, (segs, pad) in enumerate(rows):
        i, m, g = _qrow(S, segs, pad, k)
        ids.append(i); mask.append(m); grids += g
    n_slots = sum((h // Q_MERGE) * (w // Q_MERGE) for _, h, w in grids)
    slot2row = np.roll(np.arange(n_slots)[::-1], 5).astype(np.int32) if n_slots else np.zeros(0, np.int32)      # a non-identity permutation
    return types.SimpleNamespace(name=name, S=S, B=len(rows), ids=np.array(ids, np.int64), mask=np.array(mask, np.int64), grid_thw=grids,
                                 imgs=qwen_imgs(grids, Q_MERGE), slot2row=slot2row, n_slots=n_slots, clamp=False)


def make_qwen_clamped(which):
    """Batches the host wrapper refuses, which the kernel must still survive by clamping: 'runs' = more runs than images, 'long' = a run
    longer than its image (and, for the last image, than the slot table)."""
    S = 70
    if which == "runs":
        rows = [([("t", 2), ("i", 2, 2), ("t", 3), ("i", 2, 2), ("t", 5)], "left"), ([("i", 2, 2), ("t", 60), ("i", 2, 2)], "left"), ([("t", 9)], "right")]
        keep = 2                                                  # four runs, two images
    else:
        rows = [([("t", 2), ("i", 2, 3), ("t", 3)], "left"), ([("t", 1), ("i", 3, 2), ("i", 2, 2), ("t", 50)], "left"), ([("t", 9)], "right")]
        keep = 2                                                  # row 1's run holds 10 slots of a 6-slot image
    ids, mask, grids = [], [], []
    for k, (segs, pad) in enumerate(rows):
        i, m, g = _qrow(S, segs, pad, k)
        ids.append(i); mask.append(m); grids += g
    grids = grids[:keep]
    n_slots = sum((h // Q_MERGE) * (w // Q_MERGE) for _, h, w in grids)
    return types.SimpleNamespace(name="clamp_" + which, S=S, B=3, ids=np.array(ids, np.int64), mask=np.array(mask, np.int64), grid_thw=grids,
                                 imgs=qwen_imgs(grids, Q_MERGE), slot2row=np.roll(np.arange(n_slots)[::-1], 3).astype(np.int32), n_slots=n_slots, clamp=True)


def qwen_run(P, mutant=None):
    return qwen_plan_ref(P.ids, P.mask, P.grid_thw, Q_MERGE, Q_IMAGE, Q_CA, P.slot2row, mutant, clamp=P.clamp)


# ---------------------------------------------------------------------------------------------------------------------------------------
# RoPE tables
# ---------------------------------------------------------------------------------------------------------------------------------------
def f32(v):
    return torch.tensor(v, dtype=F32).item()


def ulp32(x):
    """One fp32 unit in the last place of |x| (fp64 tensor), 0 for 0."""
    _, e = torch.frexp(x.abs())
    return torch.where(x != 0, torch.exp2(e.double() - 24), torch.zeros_like(x))


def _table(ang32, scaling, swapped=False):
    """cs [..., 2] fp64 and its bound from fp32 angles: fp64 cos / sin of the fp32 value, times scaling."""
    a = ang32.double()
    c, s = torch.cos(a), torch.sin(a)
    if swapped:
        c, s = s, c
    v = torch.stack([c, s], dim=-1)
    E = TRIG_ULP * ulp32(v) * abs(scaling)
    y = v * scaling
    if scaling != 1.0:
        E = E + U32 * y.abs()
    return y, E


def use_long(seq_len, orig_max, mutant=None):
    """The module's factor choice (modeling_phi3_v.py:449): long factors iff the seq_len it is called with exceeds original_max."""
    return seq_len >= orig_max if mutant == "switch_at_ge" else seq_len > orig_max


def rope_table_ref(pos, S, inv_s, inv_l, scaling, orig_max, rotary_seq_len=0, mutant=None, mask=None):
    """cs [rows, half, 2] fp64 and its bound.  pos: int [rows]; inv_s / inv_l: fp32 tensors [half]; scaling: python float already
    rounded to fp32.  The factor choice follows the seq_len argument (rotary_seq_len, or S when 0), never the positions."""
    seq = rotary_seq_len if rotary_seq_len > 0 else S
    if mutant == "long_by_valid_length":
        seq = int(mask.sum(axis=-1).max()) if mask is not None else int(np.max(pos)) + 1
    inv = inv_l if use_long(seq, orig_max, mutant) else inv_s
    ang = torch.tensor(np.asarray(pos), dtype=torch.int64).to(F32)[:, None] * inv.to(F32)[None, :]        # one fp32 rounding
    return _table(ang, 1.0 if mutant == "scaling_dropped" else scaling, mutant == "sin_cos_swapped")


def mrope_table_ref(pos3, inv, s0, s1, mutant=None):
    """cs [rows, half, 2]: frequency k takes stream 0 for k < s0, 1 for k < s0 + s1, else 2.  pos3: int [3, rows]."""
    half = inv.numel()
    d = 1 if mutant == "mrope_stream_boundary_off_by_one" else 0
    stream = torch.tensor([0 if k < s0 + d else (1 if k < s0 + s1 + d else 2) for k in range(half)])
    p = torch.tensor(np.asarray(pos3), dtype=torch.int64).to(F32)           # [3, rows]
    ang = p[stream, :].t() * inv.to(F32)[None, :]
    return _table(ang, 1.0, mutant == "sin_cos_swapped")


def vit_rope_table_ref(hw, inv, quarter, half_pad, mutant=None):
    """cs [rows, half_pad, 2]: h * inv[k] for k < quarter, w * inv[k - quarter] for k < 2 quarter, then exact (1, 0) pairs."""
    hwt = torch.tensor(np.asarray(hw), dtype=torch.int64).to(F32)           # [rows, 2]
    rows = hwt.shape[0]
    y = torch.zeros(rows, half_pad, 2, dtype=F64)
    E = torch.zeros(rows, half_pad, 2, dtype=F64)
    if mutant != "pad_pair_zero":
        y[:, :, 0] = 1.0
    iv = inv.to(F32)
    wi = torch.arange(quarter)
    if mutant == "vit_w_uses_inv_k":
        wi = (wi + quarter).clamp_max(iv.numel() - 1)
    ang = torch.cat([hwt[:, :1] * iv[None, :quarter], hwt[:, 1:] * iv[wi][None, :]], dim=1)
    y[:, :2 * quarter], E[:, :2 * quarter] = _table(ang, 1.0, mutant == "sin_cos_swapped")
    return y, E


def table_ratio(got, y, E):
    """max |got - y| / E, an error on an exact element (E == 0) counting as infinite."""
    err = (got.double() - y).abs()
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
    r = torch.where(E > 0, err / E.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def table_emulate(ang32, scaling):
    """The fp32 evaluation cosf(ang) * scaling on the CPU (torch's fp32 cos / sin stand in for the device's)."""
    sc = torch.tensor(scaling, dtype=F32)
    return torch.stack([torch.cos(ang32) * sc, torch.sin(ang32) * sc], dim=-1)


ROPE_POS = (0, 1, 7, 8, 4095, 4096, 131071)
ROPE_ORIG_MAX = 8


def su_scaling(max_pos=131072, orig_max=ROPE_ORIG_MAX):
    """modeling_phi3_v.py:468-472, rounded to fp32 as the float argument of the entry point."""
    import math
    scale = max_pos / orig_max
    return f32(1.0 if scale <= 1.0 else math.sqrt(1 + math.log(scale) / math.log(orig_max)))


def rope_inv(head_dim, theta=10000.0):
    """(inv_short, inv_long) fp32 from synth.default_rope_factors with the reference's own torch ops (engine.rope_inv_freq)."""
    from llava_reward_amd import synth
    from llava_reward_amd.engine import rope_inv_freq
    return (rope_inv_freq(synth.default_rope_factors(head_dim, 1.0, 0.004), head_dim, theta),
            rope_inv_freq(synth.default_rope_factors(head_dim, 1.0, 0.8), head_dim, theta))


def rope_table_cases():
    """(half, B, S, rotary_seq_len, scaling kind): S = 8 and 9 around orig_max = 8 under rotary_seq_len 0, S and S + 1 (B = 2: 16 and 18
    rows), and tables of B * S = 12 rows (S = 4 and 12) whose factor choice comes from rotary_seq_len 8 / 9 or from S alone."""
    out = []
    for half in (48, 64):
        for S in (8, 9):
            for rot in (0, S, S + 1):
                out.append((half, 2, S, rot, "su" if (S + rot + half) % 2 else "one"))
        out += [(half, 3, 4, 9, "su"), (half, 1, 12, 0, "one"), (half, 3, 4, 8, "one"), (half, 1, 12, 8, "su")]
    return out


def make_rope_table(half, B, S, rot, kind):
    rows = B * S
    pos = np.array([ROPE_POS[(r + half) % len(ROPE_POS)] for r in range(rows)], np.int32)
    inv_s, inv_l = rope_inv(2 * half)
    mask = np.ones((B, S), np.int64)
    mask[:, : S // 2] = 0                                         # fewer valid tokens than S in every row: the choice must not follow them
    return types.SimpleNamespace(half=half, B=B, S=S, rot=rot, pos=pos, inv_s=inv_s, inv_l=inv_l, scaling=su_scaling() if kind == "su" else 1.0,
                                 orig_max=ROPE_ORIG_MAX, mask=mask)


def rope_table_run(P, mutant=None):
    return rope_table_ref(P.pos, P.S, P.inv_s, P.inv_l, P.scaling, P.orig_max, P.rot, mutant, P.mask)


def mrope_cases():
    return [(64, 16, 24, 7), (64, 0, 0, 5), (8, 2, 3, 9)]


def make_mrope(half, s0, s1, rows):
    g = np.random.default_rng(half + s0)
    pos3 = np.stack([g.integers(0, 40, rows), g.integers(100, 3000, rows), g.integers(5000, 140000, rows)]).astype(np.int32)   # three streams that differ
    pos3[:, 0] = (0, 1, 2)
    inv = rope_inv(2 * half, 1000000.0)[0] if half == 64 else (1.0 / (10000.0 ** (torch.arange(0, 2 * half, 2).float() / (2 * half))))
    return types.SimpleNamespace(half=half, s0=s0, s1=s1, rows=rows, pos3=pos3, inv=inv.to(F32))


def vit_cases():
    return [(20, 48, 9), (8, 16, 5)]


def make_vit(quarter, half_pad, rows):
    hw = np.array([((37 * r) % 201, (r * 2) % 4) for r in range(rows)], np.int32)
    hw[0], hw[-1] = (200, 3), (0, 0)
    inv = 1.0 / (10000.0 ** (torch.arange(0, 2 * quarter, 2).float() / (2 * quarter)))
    return types.SimpleNamespace(quarter=quarter, half_pad=half_pad, rows=rows, hw=hw, inv=inv.to(F32))


# ---------------------------------------------------------------------------------------------------------------------------------------
# rope_split
# ---------------------------------------------------------------------------------------------------------------------------------------
def _round(v32, dt):
    """fp32 -> operand type as Op<OT>::from_f32 (f16 saturates at 65504)."""
    if dt == "f16":
        v32 = v32.clamp(-F16_MAX, F16_MAX)
    return v32.to(TDT[dt])


def _encode(v32, dt, prec, mutant=None):
    """[hi] or [hi | lo] in the operand type from fp32 values (csrc/common.h split2): lo = round(v - hi) in fp32 arithmetic."""
    hi = _round(v32, dt)
    if not prec:
        return hi
    base = hi.float()
    if mutant == "lo_of_unrounded_hi":                            # the residual against v cut (not rounded) to the operand type
        m, ex = torch.frexp(v32.double())
        bits = 8 if dt == "bf16" else 11
        base = torch.ldexp(torch.trunc(torch.ldexp(m, torch.full_like(ex, bits))), ex - bits).float()
    return torch.cat([hi, _round(v32 - base, dt)], dim=1)


def _rotate(x, y, c, s, fma=False):
    """fp32 (x c - y s, y c + x s): two rounded products and one rounded sum each; fma: one product kept exact (a contracted a*b - c*d)."""
    if fma:
        return (x.double() * c.double() - (y * s).double()).float(), (y.double() * c.double() + (x * s).double()).float()
    return x * c - y * s, y * c + x * s


def rope_split_ref(qkv, cs, rope_cols, v_cols, hd, dt, prec, mutant=None):
    """The output [rows, (rope_cols + v_cols) << prec] in the operand type.  qkv fp32 [rows, rope_cols + v_cols], cs fp32 [rows, hd/2, 2]."""
    rows, half = qkv.shape[0], hd // 2
    rc = rope_cols + (v_cols if mutant == "v_rotated" else 0)     # columns that are rotated, in pairs (2p, 2p + 1)
    x, y = qkv[:, 0:rc:2], qkv[:, 1:rc:2]
    i = torch.arange(rc // 2) % half                              # pair p of a row belongs to frequency p % half of its head
    c, s = cs[:, i, 0], cs[:, i, 1]
    if mutant == "table_index_per_column_not_per_head":           # pair p reads table entry p, not p % half: past the row's table
        flat = cs.reshape(-1, 2)
        idx = (torch.arange(rows)[:, None] * half + torch.arange(rc // 2)[None, :]).clamp_max(flat.shape[0] - 1)
        c, s = flat[idx, 0], flat[idx, 1]
    ox, oy = _rotate(x, y, c, s, mutant == "fused_multiply_add")
    out = torch.cat([torch.stack([ox, oy], dim=-1).reshape(rows, rc), qkv[:, rc:]], dim=1)
    return _encode(out, dt, prec, mutant)


def rotate_half_ref(q, cos, sin):
    """modeling_phi3_v.py:521-553 on the reference's own layout (dims i and i + hd/2): q cos + rotate_half(q) sin, fp32.
    q [rows, heads, hd]; cos / sin [rows, hd/2]."""
    c, s = torch.cat([cos, cos], dim=-1)[:, None, :], torch.cat([sin, sin], dim=-1)[:, None, :]
    h = q.shape[-1] // 2
    rot = torch.cat([-q[..., h:], q[..., :h]], dim=-1)
    return q * c + rot * s


def interleave(q):
    """Reference head layout (i, i + hd/2) -> the engine's pair-interleaved layout (2i, 2i + 1)."""
    h = q.shape[-1] // 2
    return torch.stack([q[..., :h], q[..., h:]], dim=-1).reshape(q.shape)


RS_FAMILIES = ("normal", "outlier", "exact")


def rope_split_cases():
    """(rows, hd, rope_cols, v_cols, family): every hd, rope_cols in {hd, 768, 2304} (the last: more than 256 float4, two sweeps), v_cols in
    {0, 4, 1028}, rows 1 and 3; both types and both precisions run on each."""
    out = []
    k = 0
    for hd in (8, 64, 96, 128):
        for rc in (hd, 768, 2304):
            if rc % hd:
                continue
            out.append((1 if k % 2 else 3, hd, rc, (0, 4, 1028)[k % 3], RS_FAMILIES[k % 3]))
            k += 1
    out += [(3, 96, 96, 1028, "normal"), (1, 128, 2304, 0, "outlier"), (3, 64, 2304, 4, "exact"), (3, 8, 8, 0, "outlier"), (1, 8, 768, 1028, "normal")]
    return out


def make_rope_split(rows, hd, rope_cols, v_cols, family, seed=0):
    g = torch.Generator().manual_seed(seed * 101 + rows + 3 * hd + rope_cols + v_cols)
    n, half = rope_cols + v_cols, hd // 2
    if family == "exact":                                         # small integers times dyadic (cos, sin): every product and sum is exact in fp32
        qkv = torch.randint(-16, 17, (rows, n), generator=g).float()
        cs = torch.randint(-8, 9, (rows, half, 2), generator=g).float() / 8
    else:
        qkv = torch.randn(rows, n, generator=g)
        ang = torch.rand(rows, half, generator=g) * 6.3
        cs = torch.stack([torch.cos(ang), torch.sin(ang)], dim=-1) * 1.19
        if family == "outlier":
            qkv[:, ::7] *= 3.0e4 / 4                                # large values (f16 stays finite after the rotation) beside small ones
            qkv[:, 3::11] *= 2.0 ** -18
    return types.SimpleNamespace(rows=rows, hd=hd, rope_cols=rope_cols, v_cols=v_cols, family=family, qkv=qkv, cs=cs.contiguous())


def rope_split_refused(hd, rope_cols, v_cols):
    return hd % 8 != 0 or rope_cols % hd != 0 or v_cols % 4 != 0

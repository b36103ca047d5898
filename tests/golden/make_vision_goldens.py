#!/usr/bin/env python3
"""Source-map fixtures of the vision plans and gathers, recorded from the REAL programs in the build container.

Every program is fed features whose value is their own flat index (exact in fp32 below 2^24) and separators with negative labels, so its
output says, per output row, which source token landed there.  The files hold that recorded data and the program versions, nothing else.

  vision_hd_transform.npz   the reference tree's own Phi3ImageEmbedding.hd_feature_transform (modeling_phi3_v.py:254-362) at its 24 x 24 x
                            1024 with an identity projection: per crop grid an int32 [rows, 4] = source crop * 576 + token of each of the
                            four 1024-blocks, -1 for sub_GN, -2 for glb_GN, stored as row-to-row differences (cumsum over the rows
                            restores it); `batch` = the two grids of HD_BATCH in one call.
  vision_llava_pack.json    the installed transformers' LlavaNextModel.pack_image_features / unpad_image / select_best_resolution: at g = 4
                            (image_size 56, pinpoints scaled to 56) the source row (crop * 16 + token, -1 = image_newline) of every output
                            row; at g = 24 (gh, gw, r0, r1, c0, c1, rows) and a digest of that list.  The kept rectangle is
                            unpad_image's own cut of a coordinate map; a size at which the program raises is recorded as raising;
                            g24_reordered: the same under vision_ref.pinpoints_reordered.
  vision_qwen_window.npz    transformers.vision_utils get_vision_window_index / get_vision_position_ids: window_index, cu_window_seqlens
                            (before unique_consecutive) and the (h, w) of every patch, for the grid lists of vision_ref.qwen_fixture_cases(),
                            the cases back to back in one array per output.

    python tests/golden/make_vision_goldens.py
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "llava-reward_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from helpers import vision_ref as vr  # noqa: E402
from make_goldens import import_reference  # noqa: E402


def versions():
    import transformers
    return {"torch": torch.__version__, "transformers": transformers.__version__, "numpy": np.__version__}


# ---- Phi-3-V HD transform -------------------------------------------------------------------------------------------------------------
def hd_source_maps():
    import_reference()
    from llava_reward.models.base_mllm.phi3_v.modeling_phi3_v import Phi3ImageEmbedding

    class Identity(torch.nn.Module):                              # the stub projection: hd_feature_transform reads .bias for device / dtype
        def __init__(self):
            super().__init__()
            self.bias = torch.nn.Parameter(torch.zeros(1))

        def forward(self, x):
            return x

    G, C = 24, 1024
    emb = Phi3ImageEmbedding.__new__(Phi3ImageEmbedding)
    torch.nn.Module.__init__(emb)
    emb.hd_transform_order = "sub_glb"
    emb.img_projection = Identity()
    emb.glb_GN = torch.nn.Parameter(torch.full((1, 1, 4 * C), -2.0))
    emb.sub_GN = torch.nn.Parameter(torch.full((1, 1, 1, 4 * C), -1.0))

    def run(grids):
        ncrop = max(a * b for a, b in grids) + 1
        n = len(grids) * ncrop * G * G * C
        assert n < 2 ** 24
        feats = torch.arange(n, dtype=torch.float32).reshape(len(grids), ncrop, G * G, C)
        sizes = torch.tensor([[a * 336, b * 336] for a, b in grids])
        with torch.no_grad():
            out = emb.hd_feature_transform(feats, sizes)
        out = out.reshape(out.shape[0], 4, C)
        first = out[:, :, 0].to(torch.int64)
        sep = first < 0
        assert bool((out == out[:, :, :1] + torch.where(sep, 0, 1)[:, :, None] * torch.arange(C)).all()), "a block is not one token's channels"
        assert bool((first[~sep] % C == 0).all())
        tok = first // C                                          # flat (image, crop, token)
        # per image: crop * 576 + token, the image index dropped after checking that a row reads its own image only
        img = tok // (ncrop * G * G)
        bounds = np.cumsum([0] + [vr.hd_plan_ref(a, b, 1, G)[3] for a, b in grids])
        for i in range(len(grids)):
            rows = slice(bounds[i], bounds[i + 1])
            assert bool((img[rows][~sep[rows]] == i).all())
        m = torch.where(sep, first, tok % (ncrop * G * G)).numpy().astype(np.int32)
        return np.diff(m, axis=0, prepend=0).astype(np.int32), ncrop          # row-to-row differences (they repeat, the map itself does not compress)

    out = {}
    for a, b in vr.HD_GRIDS:
        out[f"g{a}x{b}"], _ = run([(a, b)])
    out["batch"], ncrop = run(list(vr.HD_BATCH))
    out["batch_ncrop"] = np.array(ncrop, np.int32)
    return out


# ---- LLaVA anyres packing -------------------------------------------------------------------------------------------------------------
def llava_records(crop, g, full, reordered=False):
    from transformers.models.llava_next.modeling_llava_next import LlavaNextModel, select_best_resolution, unpad_image
    pins = [list(p) for p in (vr.pinpoints_reordered(crop) if reordered else vr.pinpoints(crop))]
    me = types.SimpleNamespace(config=types.SimpleNamespace(image_grid_pinpoints=pins,
                                                            vision_config=types.SimpleNamespace(image_size=crop, patch_size=crop // g)))
    D, recs = 2, []
    for h, w in (vr.REORDERED_SIZES(crop) if reordered else vr.llava_sizes(crop)):
        bh, bw = select_best_resolution((h, w), pins)
        gh, gw = bh // crop, bw // crop
        n = (1 + gh * gw) * g * g
        feats = (torch.arange(n, dtype=torch.float32)[:, None] * D + torch.arange(D)).reshape(1 + gh * gw, g * g, D)
        rec = {"h": h, "w": w, "gh": gh, "gw": gw}
        # the kept rectangle, from unpad_image itself on a map of (y, x) coordinates; an empty extent has no position
        yx = torch.stack(torch.meshgrid(torch.arange(gh * g), torch.arange(gw * g), indexing="ij"))
        kept = unpad_image(yx, (h, w))
        rec["kept"] = [kept.shape[1], kept.shape[2]]
        if kept.numel():
            rec["r0"], rec["r1"], rec["c0"], rec["c1"] = int(kept[0].min()), int(kept[0].max()) + 1, int(kept[1].min()), int(kept[1].max()) + 1
        try:
            packed, lens = LlavaNextModel.pack_image_features(me, [feats], torch.tensor([[h, w]]), "default", image_newline=torch.tensor([-2.0, -1.0]))
            out = packed[0]
            assert int(lens[0]) == out.shape[0] and bool((out[:, 1] == out[:, 0] + 1).all())
            rows = [int(v) // D if v >= 0 else -1 for v in out[:, 0].tolist()]
            rec["rows"] = len(rows)
            rec["digest"] = vr.digest(rows)
            if full:
                rec["source"] = rows
        except Exception as ex:                                   # recorded, not worked around
            rec["raised"] = type(ex).__name__
        recs.append(rec)
    return recs


# ---- Qwen window plan -----------------------------------------------------------------------------------------------------------------
def qwen_records():
    from transformers.vision_utils import get_vision_position_ids, get_vision_window_index
    names, wis, cus, poss = [], [], [], []
    for name, grids in vr.qwen_fixture_cases().items():
        thw = torch.tensor([[1, a, b] for a, b in grids])
        wi, cu = get_vision_window_index(thw, spatial_merge_size=vr.QWEN_MERGE, window_size=vr.QWEN_WINDOW, patch_size=vr.QWEN_PATCH)
        pos = get_vision_position_ids(thw, vr.QWEN_MERGE)
        names.append(name)
        wis.append(torch.as_tensor(wi).numpy().astype(np.int32).reshape(-1))
        cus.append(torch.as_tensor(cu).numpy().astype(np.int32).reshape(-1))
        poss.append(torch.as_tensor(pos).numpy().astype(np.int32).reshape(-1, 2))
    # one array per output, the cases back to back; lengths[i] = entries of case names[i] in each
    return {"names": np.array(json.dumps(names)), "lengths": np.array([[len(a), len(b), len(c)] for a, b, c in zip(wis, cus, poss)], np.int32),
            "window_index": np.concatenate(wis), "cu_window_seqlens": np.concatenate(cus), "position_ids": np.concatenate(poss)}


def main():
    meta = np.array(json.dumps(versions()))
    np.savez_compressed(os.path.join(HERE, "vision_hd_transform.npz"), meta=meta, **hd_source_maps())
    with open(os.path.join(HERE, "vision_llava_pack.json"), "w") as f:
        json.dump({"versions": versions(), "pinpoint_grids": [list(p) for p in vr.LLAVA_PINPOINT_GRIDS],
                   "g4": {"crop": 56, "g": 4, "cases": llava_records(56, 4, True)},
                   "g24": {"crop": 336, "g": 24, "cases": llava_records(336, 24, False)},
                   "g24_reordered": {"crop": 336, "g": 24, "cases": llava_records(336, 24, False, True)}}, f, separators=(",", ":"))
    np.savez_compressed(os.path.join(HERE, "vision_qwen_window.npz"), meta=meta, **qwen_records())
    for n in ("vision_hd_transform.npz", "vision_llava_pack.json", "vision_qwen_window.npz"):
        print(n, os.path.getsize(os.path.join(HERE, n)), "bytes")


if __name__ == "__main__":
    main()

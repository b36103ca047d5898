#!/usr/bin/env python3
"""Record what the real programs answer on the case lists of tests/helpers/plan_ref.py (run in the build container only, like
make_goldens.py, whose import recipe it reuses; the files hold recorded data and the program versions, nothing else):

  plan_qwen_rope_index.json   Qwen2_5_VLModel.get_rope_index of the installed transformers on every qwen plan case
                              (mm_token_type_ids = (ids == image_token), as make_goldens.py passes them): ids, mask, grids, [3, B, S] result
  plan_su_rope_tables.json    Phi3SuScaledRotaryEmbedding.forward of the reference tree, head_dim 96, original_max_position_embeddings 8,
                              seq_len 8 and 9, positions {0, 1, 7, 8, 4095, 131071}: cos / sin as fp32 bit patterns, inv_freq, the scaling factor

    python tests/golden/make_plan_goldens.py
"""
import json
import math
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
from helpers import plan_ref as pr  # noqa: E402
from llava_reward_amd import synth  # noqa: E402
from make_goldens import import_reference  # noqa: E402


def _dump(name, obj):
    path = os.path.join(HERE, name)
    with open(path, "w") as f:
        json.dump(obj, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


def qwen_rope_index():
    import transformers
    from transformers import Qwen2_5_VLConfig, Qwen2_5_VLModel
    cfg = synth.qwen_tiny_config(vocab_size=151680, image_token_id=pr.Q_IMAGE, pad_token_id=pr.Q_PAD)
    v = cfg.vision
    assert v.merge == pr.Q_MERGE
    vcfg = dict(depth=v.depth, hidden_size=v.hidden, hidden_act="silu", intermediate_size=v.intermediate, num_heads=v.heads,
                in_channels=v.in_ch, patch_size=v.patch, spatial_merge_size=v.merge, temporal_patch_size=v.temporal_patch,
                tokens_per_second=2, window_size=v.window, out_hidden_size=cfg.hidden, fullatt_block_indexes=list(v.fullatt))
    tcfg = dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden, intermediate_size=cfg.intermediate,
                num_hidden_layers=cfg.layers, num_attention_heads=cfg.heads, num_key_value_heads=cfg.kv_heads,
                hidden_act="silu", max_position_embeddings=32768, rms_norm_eps=cfg.rms_eps, use_cache=False,
                tie_word_embeddings=False, use_sliding_window=False, sliding_window=32768, max_window_layers=cfg.layers,
                attention_dropout=0.0, pad_token_id=None,
                rope_parameters={"rope_type": "default", "rope_theta": cfg.rope_theta, "mrope_section": list(cfg.mrope_section)})
    hcfg = Qwen2_5_VLConfig(text_config=tcfg, vision_config=vcfg, image_token_id=cfg.image_token_id,
                            video_token_id=cfg.image_token_id + 1, vision_start_token_id=cfg.image_token_id - 3,
                            vision_end_token_id=cfg.image_token_id - 2)
    with torch.device("meta"):                                   # get_rope_index reads the config only: no weights are needed
        model = Qwen2_5_VLModel(hcfg)
    cases = {}
    for name in pr.qwen_cases():
        P = pr.make_qwen(name)
        ids, mask = torch.from_numpy(P.ids), torch.from_numpy(P.mask)
        thw = torch.tensor(P.grid_thw, dtype=torch.int64) if P.grid_thw else None
        pos, _ = model.get_rope_index(ids, (ids == pr.Q_IMAGE).int(), image_grid_thw=thw, attention_mask=mask)
        assert pos.shape == (3, P.B, P.S)
        cases[name] = {"ids": P.ids.tolist(), "mask": P.mask.tolist(), "grid_thw": [list(g) for g in P.grid_thw], "pos3": pos.tolist()}
    _dump("plan_qwen_rope_index.json", {"program": "transformers Qwen2_5_VLModel.get_rope_index", "transformers": transformers.__version__,
                                        "torch": torch.__version__, "image_token": pr.Q_IMAGE, "spatial_merge_size": v.merge, "cases": cases})


def su_rope_tables():
    import_reference()
    from llava_reward.models.base_mllm.phi3_v.modeling_phi3_v import Phi3SuScaledRotaryEmbedding
    head_dim, orig_max, max_pos, theta = 96, pr.ROPE_ORIG_MAX, 131072, 10000.0
    short, long_ = synth.default_rope_factors(head_dim, 1.0, 0.004), synth.default_rope_factors(head_dim, 1.0, 0.8)
    config = types.SimpleNamespace(max_position_embeddings=max_pos, rope_theta=theta, original_max_position_embeddings=orig_max,
                                   rope_scaling={"type": "su", "short_factor": list(short), "long_factor": list(long_)})
    module = Phi3SuScaledRotaryEmbedding(head_dim, config)
    positions = [0, 1, 7, 8, 4095, 131071]
    bits = lambda t: t.contiguous().view(torch.int32).tolist()
    tables = {}
    for seq_len in (8, 9):
        cos, sin = module(torch.zeros(1, dtype=torch.float32), torch.tensor([positions], dtype=torch.int64), seq_len=seq_len)
        assert cos.dtype == torch.float32 and cos.shape == (1, len(positions), head_dim)
        assert torch.equal(cos[..., : head_dim // 2], cos[..., head_dim // 2:])              # emb = cat(freqs, freqs)
        tables[str(seq_len)] = {"cos_bits": bits(cos[0, :, : head_dim // 2]), "sin_bits": bits(sin[0, :, : head_dim // 2]),
                                "inv_freq_bits": bits(module.inv_freq.float())}
    scale = max_pos / orig_max
    _dump("plan_su_rope_tables.json", {"program": "reference modeling_phi3_v.Phi3SuScaledRotaryEmbedding.forward", "torch": torch.__version__,
                                       "head_dim": head_dim, "original_max_position_embeddings": orig_max, "max_position_embeddings": max_pos,
                                       "rope_theta": theta, "short_factor": list(short), "long_factor": list(long_), "positions": positions,
                                       "scaling_factor": math.sqrt(1 + math.log(scale) / math.log(orig_max)), "tables": tables})


if __name__ == "__main__":
    torch.set_num_threads(1)
    qwen_rope_index()
    su_rope_tables()

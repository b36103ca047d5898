"""Scoring many captions of one image from a shared image-prefix cache (RewardModel.build_prefix / forward_prefixed,
scoring.score_captions) against the ordinary forward on the same rows.

The claim under test is bit-identity: forward_prefixed on rows [tail of the prefix | caption | right padding] returns the same bits as
custom_forward on the full right-padded rows with the image repeated per row -- in every operand form, with an un-merged adapter, with
layer_id, with either su-RoPE factor set.  The same rewards are then held to the oracle (fp32 reference) on the ordinary left-padded
batch with the bounds the forward tests use: strict 1e-4, default 3e-4, single-pass f16 1e-3."""
import numpy as np
import pytest
import torch

from llava_reward_amd import scoring, synth
from llava_reward_amd.model import RewardModel
from llava_reward_amd.preprocess import _load_rgb, hd_transform_batch, merge_text_and_image_slots
from oracle import phi3v_reward_oracle as orc

pytestmark = pytest.mark.gpu

TOL = {"f16x2": 1e-4, "f16x2f8": 3e-4, "f16": 1e-3}
SEED = 29


def _cfg(**kw):
    return synth.tiny_config(is_general_preference=True, value_head_dim=2, **kw)


def _one_image_batch(cfg, caption_lens, grid, common=0, max_crops=None):
    """synth_batch rows (left-padded) that all show sample 0's image; `common`: that many leading caption tokens made equal."""
    batch = synth.synth_batch(cfg, SEED, caption_lens, grid, max_crops=max_crops)
    batch["pixel_values"] = np.repeat(batch["pixel_values"][:1], len(caption_lens), axis=0).copy()
    if common:
        V = synth.num_img_tokens(336 * grid[0], 336 * grid[1])
        for b in range(len(caption_lens)):
            first = int(np.argmax(batch["attention_mask"][b]))
            batch["input_ids"][b, first + 4 + V:first + 4 + V + common] = np.arange(5, 5 + common)
    return batch


def _model(cfg, dtype, **kw):
    opts = dict(max_batch=4, max_seq=512, max_crops=2)
    opts.update(kw)
    if dtype == "f16x2f8":
        opts.setdefault("calibrate", False)              # the default form, as test_e4m3_residual_pass_on_tiny_config runs it
    return RewardModel(cfg, synth_seed=SEED, operand_dtype=dtype, **opts).to("cuda").eval()


def _both(m, batch):
    """(rewards of custom_forward on the right-padded rows, rewards of forward_prefixed on what follows the shared part, plan)."""
    rp = synth.right_pad(batch)
    rows = [rp["input_ids"][b][rp["attention_mask"][b] == 1] for b in range(rp["input_ids"].shape[0])]
    n_prefix, n_shared = scoring.plan_shared_prefix([r.tolist() for r in rows])
    tb = {k: torch.from_numpy(v).cuda() for k, v in rp.items()}
    want = m.custom_forward(tb["input_ids"], tb["attention_mask"], tb["pixel_values"], tb["image_sizes"])[0]
    S = rp["input_ids"].shape[1]
    state = m.build_prefix(torch.from_numpy(rows[0][:n_prefix]), tb["pixel_values"][:1], tb["image_sizes"][:1], total_len=S)
    assert (state.n_prefix, state.n_shared) == (n_prefix, n_shared)
    got = m.forward_prefixed(state, tb["input_ids"][:, n_shared:], tb["attention_mask"][:, n_shared:])[0]
    torch.cuda.synchronize()
    return want.cpu(), got.cpu(), (n_prefix, n_shared), state


_ORACLE = {}


def _oracle(cfg, key, batch):
    if key not in _ORACLE:
        W = orc.weights_to_torch(synth.make_weights(cfg, SEED))
        _ORACLE[key] = orc.custom_forward(W, cfg, batch["input_ids"], batch["attention_mask"], batch["pixel_values"], batch["image_sizes"])
    return _ORACLE[key]


CASES = {
    # 317 common tokens: 4 shared tiles + a 61-token tail | 320: the tail is empty | 1049 (grid 2x3): the ping-pong attention forms
    "a": dict(lens=[7, 3, 5, 1], grid=(1, 1), common=0, plan=(317, 256), opts={}),
    "b": dict(lens=[10, 6, 8, 4], grid=(1, 1), common=3, plan=(320, 320), opts={}),
    "c": dict(lens=[9, 4], grid=(2, 3), common=0, plan=(1049, 1024), opts=dict(max_batch=2, max_seq=1280, max_crops=7)),
}


@pytest.mark.parametrize("dtype", ["f16x2", "f16x2f8", "f16"])
@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_bit_identical_to_custom_forward_and_close_to_the_oracle(case, dtype):
    c = CASES[case]
    cfg = _cfg()
    batch = _one_image_batch(cfg, c["lens"], c["grid"], c["common"])
    m = _model(cfg, dtype, **c["opts"])
    want, got, plan, state = _both(m, batch)
    assert plan == c["plan"]
    assert 0 < state.nbytes <= state.cache.numel()
    assert torch.isfinite(got).all()
    assert torch.equal(got, want), (got - want).abs().max().item()
    ref = _oracle(cfg, case, batch)
    err = (got - ref).abs().max().item()
    print(f"[shared prefix {case} {dtype}] prefix {plan}, cache {state.nbytes} B, max |reward - oracle| = {err:.3e}")
    assert err < TOL[dtype]


@pytest.mark.parametrize("dtype", ["f16x2", "f16x2f8", "f16"])
def test_unmerged_adapter(dtype):
    cfg = _cfg(lora_rank=16)
    m = _model(cfg, dtype)
    want, got, plan, _ = _both(m, _one_image_batch(cfg, [7, 3, 5, 1], (1, 1)))
    assert plan == (317, 256) and torch.isfinite(got).all() and torch.equal(got, want)


def test_layer_id():
    cfg = _cfg()
    m = _model(cfg, "f16x2", layer_id=1)
    want, got, _, state = _both(m, _one_image_batch(cfg, [7, 3, 5, 1], (1, 1)))
    assert int(state.info.n_layers) == 1
    assert torch.isfinite(got).all() and torch.equal(got, want)
    full = _model(cfg, "f16x2")
    assert not torch.equal(_both(full, _one_image_batch(cfg, [7, 3, 5, 1], (1, 1)))[1], got)      # (layer_id is honoured, not ignored)


def test_long_factor_set():
    """orig_max_pos below the batch width: the rows run the long su-RoPE factors, and so must the cached keys."""
    cfg = _cfg(orig_max_pos=300)
    m = _model(cfg, "f16x2")
    want, got, _, state = _both(m, _one_image_batch(cfg, [7, 3, 5, 1], (1, 1)))
    assert state.long_factors
    assert torch.isfinite(got).all() and torch.equal(got, want)


# (dtype, precision map, site overrides) that put two operand forms into ONE cache.  layers: layer 0 keeps the descriptor's split
# operands, layer 1 runs a single pass -- two row widths, the cache's per-layer stride follows the attention site.  sites: every layer in
# the default form with its attention site strict while the qkv site that writes the cached rows stays default.
MIXED = {
    "layers": ("f16x2", (-1, 0, 1, 0), ()),
    "sites": ("f16x2f8", (-1, 2, 0, 0), (2, 1, 2, 2, 2)),
}


@pytest.mark.parametrize("mix", ["layers", "sites"])
def test_mixed_operand_forms_in_one_cache(mix):
    dtype, pmap, sites = MIXED[mix]
    c = CASES["a"]
    cfg = _cfg()
    batch = _one_image_batch(cfg, c["lens"], c["grid"], c["common"])
    m = _model(cfg, dtype, calibrate=False)
    eng = m.engine
    plain = _both(m, batch)[3]                                       # a state built under the map the model came with
    eng.set_precision_map(*pmap)                                     # the mixed map, BEFORE build_prefix
    eng.set_precision_sites(*sites)
    want, got, plan, state = _both(m, batch)
    assert plan == c["plan"]
    assert torch.isfinite(got).all()
    assert torch.equal(got, want), (got - want).abs().max().item()
    if mix == "layers":
        assert state.nbytes < plain.nbytes                           # (layer 1's rows are half as wide)
    rp = synth.right_pad(batch)
    ids, mask = (torch.from_numpy(rp[k][:, plan[1]:]).cuda() for k in ("input_ids", "attention_mask"))
    with pytest.raises(Exception, match="stale prefix cache"):       # each state is refused under the other map
        m.forward_prefixed(plain, ids, mask)
    eng.set_precision_sites()
    eng.set_precision_map(-1, -1, 0, 0)
    with pytest.raises(Exception, match="stale prefix cache"):
        m.forward_prefixed(state, ids, mask)


# ---- score_captions: prompts built as inference_process_phi3v builds them, from an image ----
def _rows_of(tok, image, captions, num_crops=1):
    pix, sizes, ntok = hd_transform_batch([_load_rgb(image)], num_crops, "cuda")
    rows = []
    for cap in captions:
        msg = {"role": "user", "content": f"<|image_1|>\n{cap}"}
        prompt = tok.apply_chat_template([msg], tokenize=False, add_generation_prompt=True)[:-22] + tok.eos_token
        rows.append(merge_text_and_image_slots(tok, prompt, [ntok[0]])[0][0])
    return pix, sizes, rows


def _right_padded_forward(m, pix, sizes, rows, pad=0):
    S = max(len(r) for r in rows)
    ids = torch.full((len(rows), S), pad, dtype=torch.long)
    mask = torch.zeros((len(rows), S), dtype=torch.long)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r
        mask[i, :len(r)] = 1
    out = m.custom_forward(ids.cuda(), mask.cuda(), pix.expand(len(rows), -1, -1, -1, -1).contiguous(), sizes.expand(len(rows), -1).contiguous())[0]
    torch.cuda.synchronize()
    return out.float().cpu()


def test_score_captions_order_duplicates_and_bits():
    cfg = _cfg()
    m = _model(cfg, "f16x2")
    tok = synth.StandInTokenizer()
    image = synth.synth_image(SEED, "captions", 200, 300, True)
    caps = ["a red kite", "two dogs on a beach at dusk", "x", "a red kite", "rain"]
    got = scoring.score_captions(m, tok, image, caps, num_crops=1, batch_size=2, pad_token_id=0).cpu()
    assert got.shape == (5, 2) and got.dtype == torch.float32 and torch.isfinite(got).all()
    assert torch.equal(got[0], got[3])                               # the duplicated caption, scored in different batches
    assert len({tuple(r.tolist()) for r in got}) == 4                # the others differ
    pix, sizes, rows = _rows_of(tok, image, caps)
    assert scoring.plan_shared_prefix(rows)[1] >= 64
    for i, r in enumerate(rows):                                     # every row alone, right-padded (no padding at all), in input order
        assert torch.equal(_right_padded_forward(m, pix, sizes, [r])[0], got[i]), i


def test_score_captions_rebuilds_the_prefix_across_the_rope_switch(monkeypatch):
    """Batches whose widths straddle orig_max_pos: the first runs the short factor set, the second the long one; score_captions builds
    the prefix once per set and every batch stays bit-identical to custom_forward on its rows."""
    tok = synth.StandInTokenizer()
    image = synth.synth_image(SEED, "captions", 200, 300, True)
    caps = ["ab", "abcde", "a much longer caption", "a longer caption too"]
    pix, sizes, rows = _rows_of(tok, image, caps)
    w0, w1 = max(len(r) for r in rows[:2]), max(len(r) for r in rows[2:])
    cfg = _cfg(orig_max_pos=(w0 + w1) // 2)
    assert w0 <= cfg.orig_max_pos < w1
    m = _model(cfg, "f16x2")
    built = []
    real = m.build_prefix
    monkeypatch.setattr(m, "build_prefix", lambda *a, **k: built.append(k.get("total_len")) or real(*a, **k))
    got = scoring.score_captions(m, tok, image, caps, num_crops=1, batch_size=2, pad_token_id=0).cpu()
    assert built == [w0, w1]
    want = torch.cat([_right_padded_forward(m, pix, sizes, rows[:2]), _right_padded_forward(m, pix, sizes, rows[2:])])
    assert torch.isfinite(got).all() and torch.equal(got, want)


# ---- refusals ----
def _state_and_rows(m, cfg):
    batch = synth.right_pad(_one_image_batch(cfg, [7, 3], (1, 1)))
    tb = {k: torch.from_numpy(v).cuda() for k, v in batch.items()}
    state = m.build_prefix(tb["input_ids"][0, :317], tb["pixel_values"][:1], tb["image_sizes"][:1], total_len=tb["input_ids"].shape[1])
    return state, tb["input_ids"][:, 256:], tb["attention_mask"][:, 256:]


def test_refuses_mean_hidden_state():
    cfg = _cfg()
    m = _model(cfg, "f16", mean_hidden_state=True, max_batch=2)
    with pytest.raises(Exception, match="mean_hidden_state"):
        m.build_prefix(torch.zeros(128, dtype=torch.long), torch.zeros(1, 2, 3, 336, 336), torch.tensor([[336, 336]]))


def test_refuses_a_llava_model():
    cfg = synth.llava_tiny_config()
    m = RewardModel(cfg, synth_seed=SEED, max_batch=1, max_seq=1024, max_crops=5, operand_dtype="f16").to("cuda").eval()
    with pytest.raises(NotImplementedError, match="llava"):
        m.build_prefix(torch.zeros(128, dtype=torch.long), torch.zeros(1, 5, 3, 336, 336), torch.tensor([[336, 336]]))
    import ctypes as C
    from llava_reward_amd import _lib as L
    info = L.PrefixInfo()                                            # the engine itself refuses too, by name
    rc = m.engine.lib.lr_forward_prefixed(m.engine.h, C.c_void_p(1), C.byref(info), C.c_void_p(1), C.c_void_p(1), 1, 1, 0, C.c_void_p(1), None)
    assert rc != 0 and b"LLaVA" in m.engine.lib.lr_last_error(m.engine.h)


def test_refuses_a_stale_state_and_an_oversize_batch():
    cfg = _cfg()
    m = _model(cfg, "f16x2", max_batch=2, max_seq=330)
    state, ids, mask = _state_and_rows(m, cfg)
    ok = m.forward_prefixed(state, ids, mask)[0]
    assert torch.isfinite(ok).all()
    # n_shared + T > max_seq
    wide = torch.zeros(2, 330 - 256 + 1, dtype=torch.long, device="cuda")
    with pytest.raises(Exception, match="max_seq"):
        m.forward_prefixed(state, wide, torch.ones_like(wide))
    # the operand forms moved
    m.engine.set_precision_map(0, 0, 0, 0)
    with pytest.raises(Exception, match="stale prefix cache.*operand forms"):
        m.forward_prefixed(state, ids, mask)
    m.engine.set_precision_map(-1, -1, 0, 0)
    assert torch.equal(m.forward_prefixed(state, ids, mask)[0], ok)  # (back in the form it was built in: served again)
    # a weight re-upload
    name = "model.norm.weight"
    m.engine.upload(name, torch.from_numpy(synth.make_weights(cfg, SEED)[name]))
    with pytest.raises(Exception, match="stale prefix cache.*weights"):
        m.forward_prefixed(state, ids, mask)

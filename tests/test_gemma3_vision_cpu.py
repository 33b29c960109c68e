"""Gemma-3 image input on the CPU against the installed ``transformers``
(``Gemma3ForConditionalGeneration``, ``Gemma3ImageProcessorPil``) on a tiny random model:
config mapping, preprocessing, SigLIP tower + projector, the per-row key limits of
``reference.prefill_attention`` against HF's block mask, engine greedy tokens and log-probs
(one and two images, chunk sizes that would cut an image block, a prefix-cache hit that ends
inside a block), the chat endpoint with a ``data:`` URL and TP = 2 on gloo.

Geometry: image 56, patch 14 (a 4 x 4 grid pooled 2 x 2 to 4 tokens per image), 2 tower
layers; text model with 4 layers (sliding, global, sliding, global), window 8.

The prompts are random (numpy ``default_rng(100 + seed)``). ``PROMPT_SEEDS`` = (2, 0): with the
image blocks' limits forced off (plain causal prefill, no prefix cache) the one-image prompt
of seed 2 leaves HF's greedy tokens at the first generated token and the two-image prompt of
seed 0 at the second (of seeds 0..7, one image: 1 and 6 do not move; two images: 1, 4 and 7
do not). ``test_causal_only_mask_changes_tokens`` repeats that check, so the parity tests do
see the bidirectional blocks.
"""
import base64
import io
import json

import numpy as np
import pytest
import torch

transformers = pytest.importorskip("transformers")
PIL = pytest.importorskip("PIL.Image")

from hipserve.config import PRESETS, EngineConfig, ModelConfig  # noqa: E402
from hipserve.engine.llm_engine import LLMEngine  # noqa: E402
from hipserve.engine.request import SamplingParams  # noqa: E402
from hipserve.multimodal import MultiModalPrompt, expand_image_tokens, mm_state, preprocess_image  # noqa: E402
from hipserve.ops import reference as ref  # noqa: E402
from hipserve.parallel.comm import TPGroup  # noqa: E402

IMG, BOI, EOI = 300, 302, 303
MM_TOKENS, WINDOW = 4, 8
PROMPT_SEEDS = (2, 0)      # of the one-image and of the two-image prompt
N_NEW = 8


def _hf_config():
    tc = dict(hidden_size=64, num_hidden_layers=4, num_attention_heads=4, num_key_value_heads=2, head_dim=16,
              intermediate_size=128, vocab_size=400, max_position_embeddings=512, rms_norm_eps=1e-6,
              sliding_window=WINDOW, layer_types=["sliding_attention", "full_attention"] * 2,
              query_pre_attn_scalar=16)
    vc = dict(hidden_size=32, intermediate_size=64, num_hidden_layers=2, num_attention_heads=2, image_size=56,
              patch_size=14, num_channels=3, vision_use_head=False, hidden_act="gelu_pytorch_tanh",
              layer_norm_eps=1e-6)
    return transformers.Gemma3Config(text_config=tc, vision_config=vc, mm_tokens_per_image=MM_TOKENS,
                                     boi_token_index=BOI, eoi_token_index=EOI, image_token_index=IMG,
                                     attn_implementation="eager")


def _hf_model(path):
    """Norm weights off their init, tower weights scaled up, a random projector (HF
    initialises it to zero: image rows would all be zero) and sharp attention (q_proj x 8),
    so that which keys a row sees decides the tokens."""
    torch.manual_seed(7)
    m = transformers.Gemma3ForConditionalGeneration(_hf_config()).eval()
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(torch.randn_like(p) * 0.1)
            elif name.endswith("mm_input_projection_weight"):
                p.normal_(0.0, 0.3)
            elif "vision_tower" in name or "multi_modal" in name:
                p.mul_(3.0)
            elif name.endswith("q_proj.weight"):
                p.mul_(8.0)
    m.save_pretrained(path, safe_serialization=True)
    return m


@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("gemma3mm") / "tiny")
    return _hf_model(path), path


def _engine(path, chunk=64, **kw):
    return LLMEngine(EngineConfig(model=path, device="cpu", dtype="float32", max_num_seqs=4,
                                  max_num_batched_tokens=chunk, num_kv_blocks=128, max_model_len=256, **kw),
                     tp=TPGroup())


def _image(rng, w=50, h=60):
    return PIL.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))


def _nchw(im, vc):
    """[grid^2, 3 * patch^2] patch rows -> the [3, S, S] image HF's tower takes."""
    g, p = vc.grid, vc.patch_size
    return im.pixels.reshape(g, g, 3, p, p).transpose(2, 0, 3, 1, 4).reshape(3, g * p, g * p)


def _prompt(seed, n_images, vc):
    """(ids with the image blocks expanded, images): text, image, text(, image, text)."""
    rng = np.random.default_rng(100 + seed)
    ims = [preprocess_image(_image(rng), vc) for _ in range(n_images)]
    ids = [2] + rng.integers(4, 290, 5).tolist()
    for k in range(n_images):
        ids += [BOI, IMG, EOI] + rng.integers(4, 290, 6 if k + 1 < n_images else 3).tolist()
    return expand_image_tokens(ids, ims, vc), ims


def _hf_generate(m, ids, ims, vc, n=N_NEW):
    full = torch.tensor([ids])
    pix = torch.from_numpy(np.stack([_nchw(i, vc) for i in ims]))
    with torch.no_grad():
        out = m.generate(input_ids=full, pixel_values=pix, token_type_ids=(full == IMG).long(),
                         attention_mask=torch.ones_like(full), max_new_tokens=n, do_sample=False)
    return out[0, len(ids):].tolist()


def _hf_logits(m, seq, ims, vc):
    full = torch.tensor([seq])
    pix = torch.from_numpy(np.stack([_nchw(i, vc) for i in ims]))
    with torch.no_grad():
        return m(input_ids=full, pixel_values=pix, token_type_ids=(full == IMG).long()).logits[0].float()


def _run(eng, prompts, n=N_NEW):
    """[(tokens, chosen-token log-probs)] of greedy generation, as tests/test_gemma2_cpu.py."""
    sp = SamplingParams(temperature=0.0, max_tokens=n, ignore_eos=True)
    rids = [eng.add_request(None, p, sp).request_id for p in prompts]
    toks, lps = {i: [] for i in rids}, {i: [] for i in rids}
    while eng.has_unfinished():
        for o in eng.step():
            toks[o.request_id].extend(o.new_token_ids)
            lps[o.request_id].append(o.logprobs[0])
    return [(toks[i], lps[i]) for i in rids]


def _check_against_hf(m, vc, prompts, res):
    for (ids, ims), (toks, lps) in zip(prompts, res):
        assert toks == _hf_generate(m, ids, ims, vc)
        lg = _hf_logits(m, ids + toks, ims, vc)
        for i, t in enumerate(toks):
            row = lg[len(ids) - 1 + i]
            assert row[t] >= row.max() - 1e-4, (i, t, int(row.argmax()), float(row.max() - row[t]))
            # fp32 on both sides; 1e-4 of per-logit noise over a 400-term log-softmax
            assert abs(lps[i] - float(torch.log_softmax(row, -1)[t])) <= 1e-3, (i, lps[i])


# ---------------------------------------------------------------- config, preprocessing
def test_config_mapping(ckpt):
    m, path = ckpt
    with open(f"{path}/config.json") as f:
        mc = ModelConfig.from_hf_dict(json.load(f))
    v = mc.vision
    assert mc.family == "gemma3" and mc.layer_windows == (WINDOW, 0, WINDOW, 0) and mc.mrope_section == ()
    assert v is not None and v.kind == "siglip"
    assert (v.depth, v.hidden_size, v.intermediate_size, v.num_heads, v.patch_size, v.image_size) == (2, 32, 64, 2, 14, 56)
    assert (v.mm_tokens_per_image, v.vision_start_token_id, v.vision_end_token_id, v.image_token_id) == \
        (MM_TOKENS, BOI, EOI, IMG)
    assert v.grid == 4 and v.pool == 2 and v.patch_dim == 3 * 14 * 14 and v.out_hidden_size == 64
    assert v.layer_norm_eps == 1e-6 and v.head_dim == 16
    # a text-only Gemma-3 config has no tower; Qwen3-VL keeps its kind
    assert ModelConfig.from_hf_dict(m.config.text_config.to_dict()).vision is None
    assert PRESETS["qwen3-vl-30b-a3b"].vision.kind == "qwen3_vl"


@pytest.mark.parametrize("name", ["gemma-3-4b", "gemma-3-12b", "gemma-3-27b"])
def test_presets_carry_so400m(name):
    c = PRESETS[name]
    v = c.vision
    assert v.kind == "siglip" and v.out_hidden_size == c.hidden_size
    assert (v.image_size, v.patch_size, v.depth, v.hidden_size, v.intermediate_size, v.num_heads) == \
        (896, 14, 27, 1152, 4304, 16)
    assert v.mm_tokens_per_image == 256 and v.grid == 64 and v.pool == 4 and v.head_dim == 72
    assert v.mm_tokens_per_image <= c.sliding_window
    assert PRESETS["gemma-3-1b"].vision is None


def test_preprocessing_matches_hf_processor(ckpt):
    from transformers.models.gemma3.image_processing_pil_gemma3 import Gemma3ImageProcessorPil

    vc = ModelConfig.from_hf_dict(ckpt[0].config.to_dict()).vision
    proc = Gemma3ImageProcessorPil(size={"height": 56, "width": 56}, image_mean=[0.5] * 3, image_std=[0.5] * 3)
    rng = np.random.default_rng(3)
    for w, h in [(70, 45), (56, 56), (20, 200)]:
        img = _image(rng, w, h)
        mine = preprocess_image(img, vc)
        want = proc(images=[img], return_tensors="np")["pixel_values"][0]
        assert mine.grid == (1, 4, 4) and mine.num_tokens == MM_TOKENS and mine.pixels.shape == (16, 588)
        assert np.abs(_nchw(mine, vc) - want).max() < 1e-5
    grey = PIL.fromarray(rng.integers(0, 256, (30, 40), dtype=np.uint8))  # converted to RGB
    assert np.abs(_nchw(preprocess_image(grey, vc), vc) -
                  proc(images=[grey.convert("RGB")], return_tensors="np")["pixel_values"][0]).max() < 1e-5


# ---------------------------------------------------------------- tower + projector
def test_tower_and_projector_match_transformers(ckpt):
    m, path = ckpt
    eng = _engine(path)
    vis, vc = eng.runner.model.visual, eng.model_cfg.vision
    rng = np.random.default_rng(5)
    ims = [preprocess_image(_image(rng), vc) for _ in range(2)]
    emb, ds = vis.forward(torch.from_numpy(np.concatenate([i.pixels for i in ims])))
    with torch.no_grad():
        want = m.model.get_image_features(torch.from_numpy(np.stack([_nchw(i, vc) for i in ims])),
                                          return_dict=True).pooler_output
    assert ds == [] and emb.shape == (2 * MM_TOKENS, 64) and float(want.abs().max()) > 0.5
    # the tolerance of tests/test_vision.py for the Qwen3-VL tower
    torch.testing.assert_close(emb, want.reshape(emb.shape), atol=2e-4, rtol=2e-4)


def test_pool_rmsnorm_reference():
    """The projector front against HF's module arithmetic (AvgPool2d over the patch grid,
    Gemma3RMSNorm) on fp32 data."""
    torch.manual_seed(1)
    x, w = torch.randn(2 * 36, 24), torch.randn(24) * 0.2
    got = ref.vision_pool_rmsnorm(x, w, 6, 3, 1e-6)
    p = torch.nn.functional.avg_pool2d(x.view(2, 36, 24).transpose(1, 2).reshape(2, 24, 6, 6), 3)
    p = p.flatten(2).transpose(1, 2).reshape(-1, 24)
    want = p * torch.rsqrt(p.pow(2).mean(-1, keepdim=True) + 1e-6) * (1.0 + w)
    torch.testing.assert_close(got, want, atol=1e-6, rtol=1e-5)


# ---------------------------------------------------------------- attention limits
@pytest.mark.parametrize("window", [0, 6])
def test_reference_limits_match_hf_block_mask(window):
    """``reference.prefill_attention(limits=...)`` against a dense softmax whose mask is HF's:
    OR(causal, same block of ``get_block_sequence_ids_for_mask``), AND the window on sliding layers.
    Two sequences (the second without a block), one of them a chunk on cached context."""
    from transformers.models.gemma3.modeling_gemma3 import get_block_sequence_ids_for_mask

    torch.manual_seed(11)
    nq, nkv, D, bs = 4, 2, 16, 16
    # (context length, rows of this chunk, image blocks as [start, end) absolute positions)
    seqs = [(29, 21, [(10, 14), (20, 26)]), (9, 9, [])]
    nblk = sum(-(-c // bs) for c, _, _ in seqs)
    kc, vc = torch.randn(nblk, nkv, bs, D), torch.randn(nblk, nkv, D, bs)
    bt = torch.zeros(len(seqs), 2, dtype=torch.int32)
    nb = 0
    for i, (c, _, _) in enumerate(seqs):
        for j in range(-(-c // bs)):
            bt[i, j] = nb
            nb += 1
    T = sum(q for _, q, _ in seqs)
    q = torch.randn(T, nq * D)
    cu = torch.tensor([0] + list(np.cumsum([q_ for _, q_, _ in seqs])), dtype=torch.int32)
    ctx = torch.tensor([c for c, _, _ in seqs], dtype=torch.int32)
    limits = torch.empty(T, dtype=torch.int32)
    want = torch.empty(T, nq, D)
    for i, (c, ql, blocks) in enumerate(seqs):
        tt = torch.zeros(1, c, dtype=torch.long)
        for a, b in blocks:
            tt[0, a:b] = 1
        grp = get_block_sequence_ids_for_mask(tt)[0]
        pos = torch.arange(c)
        allow = (pos[None, :] <= pos[:, None]) | ((grp[:, None] == grp[None, :]) & (grp[:, None] >= 0))
        if window:
            allow &= pos[None, :] > pos[:, None] - window
        lim = pos.clone()
        for a, b in blocks:
            lim[a:b] = b - 1
        q0 = int(cu[i])
        limits[q0:q0 + ql] = lim[c - ql:]
        k, v = ref._gather_kv(kc, vc, bt[i], c)
        kf, vf = k.repeat_interleave(nq // nkv, 1), v.repeat_interleave(nq // nkv, 1)
        s = torch.einsum("qhd,nhd->hqn", q[q0:q0 + ql].view(ql, nq, D), kf) * 0.25
        s = s.masked_fill(~allow[c - ql:][None], float("-inf"))
        want[q0:q0 + ql] = torch.einsum("hqn,nhd->qhd", torch.softmax(s, -1), vf)
    got = ref.prefill_attention(q, kc, vc, bt, cu, ctx, nq, nkv, 0.25, window, 0.0, limits)
    torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-5)
    own = torch.cat([torch.arange(c - ql, c) for c, ql, _ in seqs]).to(torch.int32)
    plain = ref.prefill_attention(q, kc, vc, bt, cu, ctx, nq, nkv, 0.25, window)
    assert torch.equal(ref.prefill_attention(q, kc, vc, bt, cu, ctx, nq, nkv, 0.25, window, 0.0, own), plain)
    assert not torch.allclose(plain, want, atol=1e-3)


# ---------------------------------------------------------------- engine against HF
@pytest.mark.parametrize("chunk", [64, 8, 5])
def test_engine_greedy_and_logprobs_match_transformers(ckpt, chunk):
    """One image, two images and a text prompt in one batch; chunk 8 and 5 would end a chunk
    inside a 4-token image block (the scheduler trims it back to the block's start)."""
    m, path = ckpt
    eng = _engine(path, chunk)
    vc = eng.model_cfg.vision
    prompts = [_prompt(PROMPT_SEEDS[0], 1, vc), _prompt(PROMPT_SEEDS[1], 2, vc)]
    text = [2, 7, 9, 33, 70, 100, 4, 250, 17, 64, 3, 90]
    res = _run(eng, [MultiModalPrompt(*p) for p in prompts] + [text])
    _check_against_hf(m, vc, prompts, res[:2])
    with torch.no_grad():
        want = m.generate(input_ids=torch.tensor([text]), attention_mask=torch.ones(1, len(text), dtype=torch.long),
                          max_new_tokens=N_NEW, do_sample=False)[0, len(text):].tolist()
    assert res[2][0] == want


def test_causal_only_mask_changes_tokens(ckpt):
    """The same prompts with the blocks' limits forced off (plain causal prefill) do not give
    HF's tokens: the parity tests above see the feature."""
    m, path = ckpt
    eng = _engine(path, enable_prefix_caching=False)
    vc = eng.model_cfg.vision
    for seed, n in zip(PROMPT_SEEDS, (1, 2)):
        ids, ims = _prompt(seed, n, vc)
        sp = SamplingParams(temperature=0.0, max_tokens=N_NEW, ignore_eos=True)
        seq = eng.add_request(None, MultiModalPrompt(ids, ims), sp)
        seq.mm.blocks = ()
        toks = []
        while eng.has_unfinished():
            for o in eng.step():
                toks.extend(o.new_token_ids)
        assert len(toks) == N_NEW and toks != _hf_generate(m, ids, ims, vc), seed


def test_prefix_cache_hit_ending_inside_a_block(ckpt):
    """KV block size 16 and an image block at positions [14, 18): the second request's
    prefix-cache hit ends at 16, inside the block. The cached rows were computed with the
    whole block visible; the rest of the block is prefilled with its limits."""
    m, path = ckpt
    eng = _engine(path, block_size=16)
    vc = eng.model_cfg.vision
    rng = np.random.default_rng(42)
    im = preprocess_image(_image(rng), vc)
    head = [2] + rng.integers(4, 290, 12).tolist() + [BOI]
    a = expand_image_tokens(head + [IMG, EOI] + rng.integers(4, 290, 5).tolist(), [im], vc)
    b = expand_image_tokens(head + [IMG, EOI] + rng.integers(4, 290, 7).tolist(), [im], vc)
    assert a[14:18] == [IMG] * 4 and a[:19] == b[:19] and a != b
    _run(eng, [MultiModalPrompt(a, [im])])
    sp = SamplingParams(temperature=0.0, max_tokens=N_NEW, ignore_eos=True)
    seq = eng.add_request(None, MultiModalPrompt(b, [im]), sp)
    toks, lps = [], []
    while eng.has_unfinished():
        for o in eng.step():
            toks.extend(o.new_token_ids)
            lps.append(o.logprobs[0])
    assert seq.num_cached_prefix == 16
    _check_against_hf(m, vc, [(b, [im])], [(toks, lps)])
    # another image behind the same token ids: no reuse of the image rows
    other = preprocess_image(_image(rng), vc)
    s2 = eng.add_request(None, MultiModalPrompt(b, [other]), sp)
    eng.step()
    assert s2.num_cached_prefix == 0


# ---------------------------------------------------------------- scheduler, engine limits
def test_scheduler_never_cuts_a_block():
    from hipserve.engine.block_manager import BlockManager
    from hipserve.engine.request import Sequence
    from hipserve.engine.scheduler import Scheduler

    vc = PRESETS["gemma-3-4b"].vision
    vc = vc.__class__(**{**vc.__dict__, "mm_tokens_per_image": 4, "image_size": 56, "image_token_id": IMG})
    im = preprocess_image(_image(np.random.default_rng(0)), vc)
    ids = expand_image_tokens([2, 5, 6, IMG, 7, 8, 9, IMG, 3], [im, im], vc)  # blocks [3, 7) and [10, 14)

    def chunks(budget, other_decodes=0):
        sch = Scheduler(BlockManager(64, 16, False), 8, budget, 256)
        sp = SamplingParams(temperature=0.0, max_tokens=64, ignore_eos=True)
        for j in range(other_decodes):  # sequences ahead of it that take a token per step
            s = Sequence(f"d{j}", [2, 3], sp)
            sch.add(s)
        seq = Sequence("mm", list(ids), sp)
        seq.mm = mm_state(ids, [im, im], vc)
        sch.add(seq)
        got = []
        for _ in range(40):
            so = sch.schedule()
            for s in so.prefill + so.decode:
                if s.seq is seq:
                    got.append((s.start, s.end))
                s.seq.num_computed_tokens = s.end
                if not s.seq.is_prefill:
                    s.seq.append_token(5)
            if seq.num_computed_tokens >= len(ids):
                break
        return got

    assert chunks(64) == [(0, 15)]
    assert chunks(5) == [(0, 3), (3, 8), (8, 10), (10, 15)]   # 5 and 13 lie inside a block
    assert chunks(4) == [(0, 3), (3, 7), (7, 10), (10, 14), (14, 15)]
    assert chunks(6) == [(0, 3), (3, 9), (9, 15)]
    # two decoding sequences ahead leave 2 of 4 tokens: room is held for the whole block
    got = chunks(4, other_decodes=2)
    assert got[0][0] == 0 and got[-1][1] == 15 and all(b == c for (_, b), (c, _) in zip(got, got[1:]))
    for a, b in got:
        assert not any(lo < b < hi for lo, hi in [(3, 7), (10, 14)]), got


def test_engine_refuses_budgets_below_one_image(ckpt):
    _, path = ckpt
    with pytest.raises(ValueError, match="max_num_batched_tokens"):
        _engine(path, chunk=MM_TOKENS - 1)
    mc = ModelConfig.from_hf_dict(ckpt[0].config.to_dict())
    small = mc.replace(sliding_window=3, layer_windows=(3, 0, 3, 0))
    with pytest.raises(ValueError, match="sliding_window"):
        LLMEngine(EngineConfig(model="tiny-g3", load_format="dummy", device="cpu", dtype="float32", max_num_seqs=2,
                               max_num_batched_tokens=32, num_kv_blocks=32, max_model_len=64),
                  tp=TPGroup(), model_cfg=small)


def test_dummy_weights_allocate_a_tower(ckpt):
    mc = ModelConfig.from_hf_dict(ckpt[0].config.to_dict())
    eng = LLMEngine(EngineConfig(model="tiny-g3", load_format="dummy", device="cpu", dtype="float32", max_num_seqs=2,
                                 max_num_batched_tokens=32, num_kv_blocks=32, max_model_len=64),
                    tp=TPGroup(), model_cfg=mc)
    ids, ims = _prompt(1, 1, mc.vision)
    (toks, _), = _run(eng, [MultiModalPrompt(ids, ims)], n=3)
    assert len(toks) == 3 and eng.runner.model.visual.proj_w.shape == (64, 32)


# ---------------------------------------------------------------- chat surface
def test_chat_prompt_expansion(ckpt):
    from hipserve.tokenizer import SyntheticTokenizer

    vc = ModelConfig.from_hf_dict(ckpt[0].config.to_dict()).vision
    tk = SyntheticTokenizer(400)
    msgs = [{"role": "user", "content": [{"type": "text", "text": "hi"},
                                         {"type": "image_url", "image_url": {"url": "data:x"}},
                                         {"type": "text", "text": "there"}]}]
    ids, urls = tk.encode_chat_mm(msgs, vc)
    nl = tk.encode("\n\n", add_special_tokens=False)
    i = ids.index(BOI)
    assert urls == ["data:x"] and ids.count(IMG) == 1
    assert ids[i - len(nl):i] == nl and ids[i:i + 3] == [BOI, IMG, EOI] and ids[i + 3:i + 3 + len(nl)] == nl
    im = preprocess_image(_image(np.random.default_rng(2)), vc)
    full = expand_image_tokens(ids, [im], vc)
    st = mm_state(full, [im], vc)
    assert st.spans == [(i + 1, i + 1 + MM_TOKENS)] and st.blocks == ((i + 1, i + 1 + MM_TOKENS),) and st.delta == 0
    assert np.array_equal(st.pos3[0], np.arange(len(full))) and all(h < 0 for h in st.hash_ids[i + 1:i + 5])


def test_chat_endpoint_with_data_url(ckpt):
    """POST /v1/chat/completions with an image_url part: 200 and the tokens of the engine-level
    call on the same prompt; a broken image is a 400 and the engine stays alive."""
    import asyncio

    import aiohttp
    from aiohttp import web

    from hipserve.server.api_server import OpenAIServer
    from hipserve.server.async_engine import AsyncEngine

    _, path = ckpt
    buf = io.BytesIO()
    _image(np.random.default_rng(13), 96, 64).save(buf, format="PNG")
    url = "data:image/png;base64," + base64.b64encode(buf.getvalue()).decode()
    msgs = [{"role": "user", "content": [{"type": "image_url", "image_url": {"url": url}},
                                         {"type": "text", "text": "what is this"}]}]

    async def main():
        eng = _engine(path)
        ae = AsyncEngine(eng)
        ae.start(asyncio.get_running_loop())
        srv = OpenAIServer(ae, "g3", eng.max_model_len)
        prompt = await srv._encode_images(msgs, eng.model_cfg.vision)
        assert prompt.ids.count(IMG) == MM_TOKENS
        runner = web.AppRunner(srv.app())
        await runner.setup()
        site = web.TCPSite(runner, "127.0.0.1", 0)
        await site.start()
        base = f"http://127.0.0.1:{site._server.sockets[0].getsockname()[1]}"
        try:
            async with aiohttp.ClientSession() as s:
                r = await s.post(base + "/v1/chat/completions", json={
                    "model": "g3", "messages": msgs, "max_tokens": 4, "temperature": 0, "ignore_eos": True})
                j = await r.json()
                assert r.status == 200, j
                assert j["usage"]["completion_tokens"] == 4 and j["usage"]["prompt_tokens"] == len(prompt.ids)
                bad = [{"role": "user", "content": [{"type": "image_url",
                                                     "image_url": {"url": "data:image/png;base64,AAAA"}}]}]
                r = await s.post(base + "/v1/chat/completions", json={"model": "g3", "messages": bad})
                assert r.status == 400
                assert (await s.get(base + "/health")).status == 200
        finally:
            ae.stop()
            await runner.cleanup()

    asyncio.run(main())


# ---------------------------------------------------------------- TP = 2
def _tp_cfg(path, tp):
    return EngineConfig(model=path, device="cpu", dtype="float32", tensor_parallel_size=tp, num_kv_blocks=128,
                        max_model_len=256, max_num_batched_tokens=9, max_num_seqs=4)


def _tp_generate(eng):
    vc = eng.model_cfg.vision
    prompts = [MultiModalPrompt(*_prompt(PROMPT_SEEDS[1], 2, vc)), [2, 3, 4, 5, 6]]
    return [r[0] for r in eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True))]


def _tp_worker(rank, world, port, path, q):
    import os

    import torch.distributed as dist

    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    from hipserve.config import resolve_model_config
    from hipserve.engine.llm_engine import worker_loop
    from hipserve.engine.model_runner import ModelRunner
    from hipserve.parallel.comm import init_tp

    tp = init_tp(world, backend="gloo", device_type="cpu")
    cfg = _tp_cfg(path, world)
    try:
        if rank == 0:
            eng = LLMEngine(cfg, tp=tp)
            q.put(_tp_generate(eng))
            eng.shutdown()
        else:
            worker_loop(ModelRunner(cfg, resolve_model_config(path), tp), tp)
    finally:
        dist.destroy_process_group()
    q.close()
    q.join_thread()
    os._exit(0)


def test_tp2_matches_tp1(ckpt):
    """TP = 2 over gloo: the limits and the pixels travel in the step broadcast, every rank
    runs the replicated tower; the tokens are TP = 1's."""
    import socket

    import torch.multiprocessing as mp

    _, path = ckpt
    want = _tp_generate(LLMEngine(_tp_cfg(path, 1), tp=TPGroup()))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_tp_worker, args=(r, 2, port, path, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = q.get(timeout=300)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got == want

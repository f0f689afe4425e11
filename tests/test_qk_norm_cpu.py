"""Qwen3 on the CPU: the QK-norm reference op against independent torch, the model against
``transformers.Qwen3ForCausalLM`` (fp32), checkpoints, tensor parallelism, routing, refusals and
the tokenizer's BOS rule."""
import math

import pytest
import torch
import torch.nn.functional as F

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.models import (AttnMeta, CausalLM, config_from_hf, config_to_hf, get_config, load_checkpoint,
                                        save_checkpoint)
from k8s_llm_monitor_amd.ops import reference as ref

U = 2.0 ** -24  # fp32 unit roundoff (half an ulp)


def _prefill_logits(model, ids):
    n = len(ids)
    meta = AttnMeta(is_prefill=True, positions=torch.arange(n, dtype=torch.int32),
                    slot_mapping=torch.full((n,), -1, dtype=torch.int32),
                    cu_seqlens=torch.tensor([0, n], dtype=torch.int32))
    return model.forward(torch.tensor(ids, dtype=torch.int32), meta, None).float()


# ------------------------------------------------------------------ the reference op
@pytest.mark.parametrize("hq,hkv,D", [(4, 2, 64), (8, 2, 128), (3, 1, 64)])
@pytest.mark.parametrize("rope", [True, False])
def test_reference_matches_independent_torch(hq, hkv, D, rope):
    """ref.rope_and_cache(qk_norm=) in fp32 against F.rms_norm per head + the reference RoPE, both in
    fp64.  Roundings per fp32 output, each at most U = 2^-24 relative: the square (1) and the sum of
    D squares (at most ceil(log2 D) + 2 deep: vector lanes, then a tree) and + eps (1) reach the
    result through the inverse square root at half weight; then sqrt and reciprocal (2), * r and
    * w (2), and with RoPE one product and the sum (2).  With RoPE the bound is relative to
    |a cos| + |b sin| (a difference can cancel); without it, to the result itself."""
    T = 9
    g = torch.Generator().manual_seed(7)
    n = (hq + 2 * hkv) * D
    qkv = torch.randn(T, n, generator=g)
    for h in range(hq + hkv):
        qkv[:, h * D:(h + 1) * D] *= 2.0 ** (h % 5)
    qkv[4, hq * D:(hq + 1) * D] *= 1e-3  # eps matters for this k head
    eps = 1e-4
    qw, kw = torch.rand(D, generator=g) * 1.5 + 0.5, torch.rand(D, generator=g) * 1.5 + 0.5
    pos = torch.randint(0, 500, (T,), generator=g).to(torch.int32)
    cs = ref.rope_cos_sin(512, D, 1e6)
    got = qkv.clone()
    ref.rope_and_cache(got, pos, cs, None, None, None, hq, hkv, D, rope, qk_norm=(qw, kw, eps))
    assert torch.equal(got[:, (hq + hkv) * D:], qkv[:, (hq + hkv) * D:]), "v is untouched"

    x = qkv.double()
    qn = F.rms_norm(x[:, :hq * D].view(T, hq, D), (D,), qw.double(), eps)
    kn = F.rms_norm(x[:, hq * D:(hq + hkv) * D].view(T, hkv, D), (D,), kw.double(), eps)
    xn = torch.cat([qn, kn], 1)  # [T, hq + hkv, D] fp64
    nops = (1 + math.ceil(math.log2(D)) + 2 + 1) / 2 + 2 + 2 + (2 if rope else 0)
    rtol = nops * U
    if rope:
        want = ref.apply_rope(xn, pos, cs)
        assert want.dtype == torch.float64
        c = cs[pos.long()].double()
        cc, ss = c[:, None, :D // 2], c[:, None, D // 2:]
        a, b = xn[..., :D // 2].abs(), xn[..., D // 2:].abs()
        mag = torch.cat([a * cc.abs() + b * ss.abs(), b * cc.abs() + a * ss.abs()], -1)
    else:
        want, mag = xn, xn.abs()
    err = (got[:, :(hq + hkv) * D].view(T, hq + hkv, D).double() - want).abs()
    worst = float((err / mag).max())
    print(f"D {D} rope {rope}: worst err / magnitude {worst / U:.2f} U, bound {nops} U")
    assert bool((err <= rtol * mag).all()), f"worst {worst / U:.2f} U > {nops} U"


def test_cpu_op_reduces_slabs_then_norms():
    """The CPU branch of ops.rope_and_cache with ``partial``: the slab sum rounded to the row dtype,
    then the reference - the same as the reference over rows that hold the sum."""
    hq, hkv, D, T, S = 4, 2, 64, 5, 3
    g = torch.Generator().manual_seed(3)
    n = (hq + 2 * hkv) * D
    part = torch.randn(S, T, n, generator=g)
    qw, kw = torch.rand(D, generator=g) + 0.5, torch.rand(D, generator=g) + 0.5
    pos = torch.arange(T, dtype=torch.int32)
    cs = ref.rope_cos_sin(64, D, 1e6)
    k1, v1 = (t[0] for t in ops.kv_cache_alloc(1, 2, hkv, D, torch.bfloat16, "cpu"))
    k2, v2 = k1.clone(), v1.clone()
    slots = torch.tensor([3, -1, 17, 18, 0], dtype=torch.int32)
    a = torch.zeros(T, n, dtype=torch.bfloat16)
    ops.rope_and_cache(a, pos, cs, k1, v1, slots, hq, hkv, D, partial=part.reshape(-1), nslabs=S, qk_norm=(qw, kw, 1e-6))
    b = part.sum(0).to(torch.bfloat16)
    ref.rope_and_cache(b, pos, cs, k2, v2, slots, hq, hkv, D, qk_norm=(qw, kw, 1e-6))
    assert torch.equal(a, b) and torch.equal(k1, k2) and torch.equal(v1, v2)
    plain = part.sum(0).to(torch.bfloat16)
    ref.rope_and_cache(plain, pos, cs, None, None, None, hq, hkv, D)
    assert not torch.equal(a[:, :(hq + hkv) * D], plain[:, :(hq + hkv) * D]), "the norm did something"
    with pytest.raises(ValueError):
        ops.rope_and_cache(a, pos, cs, None, None, None, hq, hkv, D, qk_norm=(qw[:32], kw, 1e-6))


# ------------------------------------------------------------------ Hugging Face parity
transformers = pytest.importorskip("transformers")


def _hf_qwen3(tie: bool, **kw):
    torch.manual_seed(0)
    args = dict(vocab_size=320, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=4,
                num_key_value_heads=2, head_dim=64, max_position_embeddings=256, rope_theta=1e6, rms_norm_eps=1e-6,
                tie_word_embeddings=tie, bos_token_id=1, eos_token_id=2)
    args.update(kw)
    hf = transformers.Qwen3ForCausalLM(transformers.Qwen3Config(**args))
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # every parameter random: HF inits the norms (q / k norms too) to 1
        for n, p in hf.named_parameters():
            if p.dim() == 1:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
    return hf.float().eval()


@pytest.mark.parametrize("tie", [True, False])
def test_hf_qwen3_checkpoint_matches_transformers_forward(tmp_path, tie):
    hf = _hf_qwen3(tie)
    assert hf.config.hidden_size // hf.config.num_attention_heads != hf.config.head_dim
    assert not torch.equal(hf.model.layers[0].self_attn.q_norm.weight, hf.model.layers[0].self_attn.k_norm.weight)
    hf.save_pretrained(tmp_path / "hf", safe_serialization=True)
    cfg = config_from_hf(tmp_path / "hf")
    assert cfg.arch == "llama" and cfg.qk_norm and not cfg.add_bos and cfg.head_dim == 64
    assert cfg.tie_embeddings == tie and cfg.rope_theta == 1e6 and cfg.norm_eps == 1e-6
    m = CausalLM(cfg, device="cpu", dtype=torch.float32, init="empty")
    assert load_checkpoint(m, tmp_path / "hf") == []
    ids = [1, 17, 33, 250, 5, 99, 140, 7, 61, 200, 3, 45]
    ours = _prefill_logits(m, ids)
    with torch.no_grad():
        want = hf(torch.tensor([ids])).logits[0].float()
    err = (ours - want).abs().max().item()
    assert err < 2e-3 * max(1.0, want.abs().max().item()), f"max |logit diff| {err}"
    assert torch.equal(ours.argmax(-1), want.argmax(-1))
    # save -> load round trip, under the Qwen3 names
    assert config_to_hf(cfg)["model_type"] == "qwen3"
    save_checkpoint(m, tmp_path / "ours")
    cfg2 = config_from_hf(tmp_path / "ours")
    for f in ("vocab_size", "d_model", "n_layers", "n_heads", "n_kv_heads", "head_dim", "ffn_dim", "tie_embeddings",
              "bos_id", "eos_ids", "qk_norm", "add_bos", "rope_theta", "norm_eps", "max_position"):
        assert getattr(cfg2, f) == getattr(cfg, f), f
    b = CausalLM(cfg2, device="cpu", dtype=torch.float32, seed=99)
    load_checkpoint(b, tmp_path / "ours")
    assert torch.equal(_prefill_logits(b, ids), ours)
    # and transformers reads what save_checkpoint wrote
    back = transformers.Qwen3ForCausalLM.from_pretrained(tmp_path / "ours", torch_dtype=torch.float32).eval()
    with torch.no_grad():
        assert torch.equal(back(torch.tensor([ids])).logits[0].float(), want)


def test_cpu_engine_serves_a_transformers_qwen3_directory(tmp_path):
    """EngineConfig.weights on a directory written by Qwen3ForCausalLM.save_pretrained: paged
    prefill and decode on the CPU generate the fp32 transformers model's greedy tokens."""
    from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams

    hf = _hf_qwen3(False)
    with torch.no_grad():  # decisive logits
        for p in hf.parameters():
            if p.dim() == 2:
                p.mul_(3.0)
    hf.save_pretrained(tmp_path, safe_serialization=True)
    eng = LLMEngine(EngineConfig(weights=str(tmp_path), max_num_seqs=2, max_model_len=128, num_blocks=32,
                                 use_graphs=False, dtype="float32"), device="cpu")
    assert eng.model_cfg.qk_norm
    prompts = [[1, 17, 33, 250, 5, 99, 140, 7, 61, 200, 3, 45], [9, 300, 12, 12, 4]]
    seqs = eng.generate(prompts, SamplingParams(max_tokens=6, temperature=0.0, ignore_eos=True))
    for s, p in zip(seqs, prompts):
        with torch.no_grad():
            out = hf.generate(torch.tensor([p]), max_new_tokens=6, do_sample=False,
                              attention_mask=torch.ones(1, len(p), dtype=torch.long))[0, len(p):].tolist()
        assert s.output_ids == out


def test_seeded_weights_and_bookkeeping():
    cfg = get_config("qwen3-tiny")
    a = CausalLM(cfg, device="cpu", dtype=torch.float32, seed=5)
    L = a.layers[0]
    for k in ("q_norm", "k_norm"):
        assert L[k].shape == (cfg.head_dim,) and not torch.equal(L[k], torch.ones_like(L[k]))
        assert float((L[k] - 1).abs().max()) < 0.6
        assert a.canonical(L, k) is L[k]
    assert not torch.equal(L["q_norm"], L["k_norm"])
    assert cfg.num_params() == cfg.replace(qk_norm=False).num_params() + cfg.n_layers * 2 * cfg.head_dim
    plain = CausalLM(cfg.replace(qk_norm=False), device="cpu", dtype=torch.float32, seed=5)
    extra = cfg.n_layers * 2 * cfg.head_dim
    assert a.num_local_params() == plain.num_local_params() + extra
    assert a.resident_weight_bytes() == plain.resident_weight_bytes() + 4 * extra
    b = CausalLM(cfg, device="cpu", dtype=torch.float32, seed=6)
    assert not torch.equal(b.layers[1]["k_norm"], a.layers[1]["k_norm"])
    b.copy_weights_from(a)
    assert torch.equal(b.layers[1]["k_norm"], a.layers[1]["k_norm"])
    ids = [3, 9, 27, 81, 243, 11]
    assert torch.equal(_prefill_logits(a, ids), _prefill_logits(b, ids))
    assert not torch.equal(_prefill_logits(a, ids), _prefill_logits(plain, ids))


def test_registry():
    c = get_config("qwen3-8b")
    assert (c.n_layers, c.d_model, c.n_heads, c.n_kv_heads, c.head_dim, c.ffn_dim, c.vocab_size) == \
        (36, 4096, 32, 8, 128, 12288, 151936)
    assert c.rope_theta == 1e6 and c.norm_eps == 1e-6 and c.max_position == 40960 and not c.tie_embeddings
    assert c.qk_norm and not c.add_bos
    s = get_config("qwen3-0.6b")
    assert (s.n_layers, s.d_model, s.n_heads, s.n_kv_heads, s.head_dim, s.ffn_dim) == (28, 1024, 16, 8, 128, 3072)
    assert s.tie_embeddings and s.qk_norm
    assert get_config("qwen3-tiny").head_dim == 64
    t = get_config("qwen3-tiny-d128")
    assert (t.n_heads, t.n_kv_heads, t.head_dim) == (8, 2, 128)
    assert not get_config("llama-3-8b").qk_norm and get_config("llama-3-8b").add_bos


# ------------------------------------------------------------------ tensor parallelism
def test_tp2_matches_tp1():
    """qwen3-tiny at TP = 2 on CPU gloo against TP = 1: the forward and the engine's tokens, by
    test_parallel's worker (the q / k norm weights are whole on both ranks)."""
    import torch.multiprocessing as mp
    from test_parallel import _free_port, _worker

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, "qwen3-tiny", q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(60)
    for rank, err, vocab, toks, want in res:
        assert not isinstance(err, str), err
        assert err < 2e-3, f"rank {rank}: max |tp - ref| = {err}"
        if rank == 0:
            assert toks == want


# ------------------------------------------------------------------ routing
def test_routing():
    q = CausalLM(get_config("qwen3-tiny-d128"), device="cpu", dtype=torch.float32, seed=1)
    l = CausalLM(get_config("llama-tiny-d128"), device="cpu", dtype=torch.float32, seed=1)
    assert l._attn_rope is True and q._attn_rope is False
    assert q._skinny_ws is not None, "the decode GEMM path itself stays"
    h = torch.zeros(4096, 512)
    assert q._fused_norm_ok(h) is False
    # what keeps a QK-norm model off the fused-norm prefill is the config, not the device: the
    # same question asked of a tensor that claims to be on the GPU

    class OnGpu:
        is_cuda = True
        shape = (4096, 512)

    assert q._fused_norm_ok(OnGpu()) is False


# ------------------------------------------------------------------ refusals
_QWEN3_HF = {"model_type": "qwen3", "vocab_size": 151936, "hidden_size": 4096, "num_hidden_layers": 36,
             "num_attention_heads": 32, "num_key_value_heads": 8, "head_dim": 128, "intermediate_size": 12288,
             "max_position_embeddings": 40960, "rope_theta": 1000000.0, "rms_norm_eps": 1e-6,
             "tie_word_embeddings": False, "bos_token_id": 151643, "eos_token_id": 151645,
             "attention_bias": False, "use_sliding_window": False, "sliding_window": None, "rope_scaling": None}


def test_config_from_hf_qwen3_and_refusals():
    c = config_from_hf(dict(_QWEN3_HF))
    want = get_config("qwen3-8b")
    for f in ("vocab_size", "d_model", "n_layers", "n_heads", "n_kv_heads", "head_dim", "ffn_dim", "max_position",
              "rope_theta", "norm_eps", "qk_norm", "add_bos", "tie_embeddings"):
        assert getattr(c, f) == getattr(want, f), f
    assert c.eos_ids == (151645,)
    assert config_from_hf(dict(_QWEN3_HF, eos_token_id=[151645, 151643])).eos_ids == (151645, 151643)
    # head_dim is read, not derived: Qwen3-0.6B has 1024 / 16 = 64 but head_dim 128
    assert config_from_hf(dict(_QWEN3_HF, hidden_size=1024, num_attention_heads=16)).head_dim == 128
    for bad in ({"attention_bias": True}, {"use_sliding_window": True}, {"model_type": "qwen3_moe"},
                {"rope_scaling": {"rope_type": "yarn", "factor": 4.0, "original_max_position_embeddings": 32768}}):
        with pytest.raises(ValueError):
            config_from_hf(dict(_QWEN3_HF, **bad))
    lc = config_from_hf({"model_type": "llama", "vocab_size": 320, "hidden_size": 128, "num_hidden_layers": 1,
                         "num_attention_heads": 4, "intermediate_size": 256})
    assert not lc.qk_norm and lc.add_bos


# ------------------------------------------------------------------ tokenizer
def test_no_bos_for_qwen3_and_one_for_llama(tmp_path):
    from k8s_llm_monitor_amd.engine.tokenizer import HFTokenizer, tokenizer_for, tokenizer_from_dir

    text = "pod default/api-gateway CrashLoopBackOff"
    qc, lc = get_config("qwen3-tiny"), get_config("llama-tiny")
    qt, lt = tokenizer_for(qc), tokenizer_for(lc)
    body = lt.encode(text, bos=False)
    assert body and lc.bos_id not in body
    assert lt.encode(text) == [lc.bos_id] + body
    assert qt.encode(text) == qt.encode(text, bos=False) == body
    assert qt.decode(qt.encode(text)) == text
    for name in ("mixtral-tiny", "gpt2-tiny", "llama-3-8b"):
        c = get_config(name)
        assert tokenizer_for(c).encode(text)[0] == c.bos_id
    tokenizers = pytest.importorskip("tokenizers")
    tok = tokenizers.Tokenizer(tokenizers.models.BPE(unk_token="<unk>"))
    tok.pre_tokenizer = tokenizers.pre_tokenizers.ByteLevel(add_prefix_space=False)
    tok.decoder = tokenizers.decoders.ByteLevel()
    tok.train_from_iterator([text * 20], tokenizers.trainers.BpeTrainer(vocab_size=300,
                                                                        special_tokens=["<unk>", "<s>", "</s>"]))
    tok.save(str(tmp_path / "tokenizer.json"))
    hq, hl = tokenizer_from_dir(tmp_path, qc), tokenizer_from_dir(tmp_path, lc)
    assert isinstance(hq, HFTokenizer) and isinstance(hl, HFTokenizer)
    assert hl.encode(text) == [lc.bos_id] + hq.encode(text) and hq.encode(text) == hl.encode(text, bos=False)

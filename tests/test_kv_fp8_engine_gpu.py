"""An engine on an fp8 (e4m3) KV cache at Llama-3-8B dimensions (2 layers), graphs on, up to 128
rows per step.

The decode graphs must have captured paged_decode_fused with an e4m3 cache.  Batches of 3 and of
128 prompts are checked against the fp32 CPU model (tests/test_fp8_engine_gpu.py's reference) driven
through ``forward`` over an fp8 paged cache of its own - the prompt prefilled, then one decode step
per token the GPU emitted - so its KV is quantised at the same points as the GPU's:

* ``err``: the GPU-vs-fp32 prefill logit error of the existing rule (< 0.03 x scale);
* ``d_kv``: the max-abs logit difference between that reference and the same reference over an
  unquantised cache - the size of the quantisation effect, measured on the reference alone (> 0);
* every GPU token's reference logit is within 2 err + 2 d_kv of its row's maximum (bf16-vs-fp32
  rounding of k / v can flip individual codes, hence the d_kv term).

Measured on MI355X (profiles/r11/README.md has the printed figures)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
N_NEW = 6
CHECKED_128 = [0, 64, 127]
F8 = torch.float8_e4m3fn


def _fp32_reference(gpu_model):  # as tests/test_fp8_engine_gpu.py
    from k8s_llm_monitor_amd.models import CausalLM
    from k8s_llm_monitor_amd.parallel.state import ParallelState

    CausalLM.SKINNY_DECODE = False  # the reference runs the plain row-major path only
    try:
        ref = CausalLM(gpu_model.cfg, device="cpu", dtype=torch.float32, pstate=ParallelState(), init="empty")
    finally:
        CausalLM.SKINNY_DECODE = True
    ref.copy_weights_from(gpu_model)
    return ref


def _logits(model, ids, rows, device):
    from k8s_llm_monitor_amd.models import AttnMeta

    n = len(ids)
    t = torch.tensor(ids, dtype=torch.int32, device=device)
    meta = AttnMeta(is_prefill=True, positions=torch.arange(n, dtype=torch.int32, device=device),
                    slot_mapping=torch.full((n,), -1, dtype=torch.int32, device=device),
                    cu_seqlens=torch.tensor([0, n], dtype=torch.int32, device=device),
                    logits_idx=torch.tensor(rows, device=device))
    return model.forward(t, meta, None).float().cpu()


def _paged_logits(ref, prompt, outs, kv_dtype, chunk=None):
    """Row t = the reference's logits for output token t, computed as the engine computes them:
    the prompt prefilled (in ``chunk``-token steps, later chunks attending the earlier ones through
    the cache) into a paged cache of ``kv_dtype``, then one decode step per emitted token."""
    from k8s_llm_monitor_amd import ops
    from k8s_llm_monitor_amd.models import AttnMeta

    i32 = lambda x: torch.tensor(x, dtype=torch.int32)  # noqa: E731
    p = len(prompt)
    nb = (p + len(outs) + 15) // 16
    alloc = ops.kv_cache_alloc(ref.cfg.n_layers, nb, ref.hkv, ref.D, kv_dtype, "cpu")
    kv = [(alloc[0][i], alloc[1][i], alloc[2][i] if len(alloc) > 2 else None) for i in range(ref.cfg.n_layers)]
    bt = torch.arange(nb, dtype=torch.int32)[None]
    rows = []
    step = chunk or p
    for a in range(0, p, step):
        b = min(p, a + step)
        meta = AttnMeta(is_prefill=True, positions=torch.arange(a, b, dtype=torch.int32),
                        slot_mapping=torch.arange(a, b, dtype=torch.int32), cu_seqlens=i32([0, b - a]),
                        logits_idx=torch.tensor([b - a - 1]))
        if a:
            meta.ctx_start, meta.block_tables = i32([a]), bt
        lg = ref.forward(i32(prompt[a:b]), meta, kv).float()
    rows.append(lg)
    for t in range(len(outs) - 1):
        pos = p + t
        meta = AttnMeta(is_prefill=False, positions=i32([pos]), slot_mapping=i32([pos]), block_tables=bt,
                        seq_lens=i32([pos + 1]))
        rows.append(ref.forward(i32([outs[t]]), meta, kv).float())
    return torch.cat(rows)


def _prompts(n, tag):
    return [f"{tag} node-{i:03d} CPU={30 + i % 60}% pod payments-{i} restarts={i % 7} 为什么我的pod频繁重启？" for i in range(n)]


def _cfg(seed=5, **kw):
    from k8s_llm_monitor_amd.engine import EngineConfig

    kw.setdefault("prefix_caching", False)
    return EngineConfig(model="llama-3-8b", model_overrides={"n_layers": 2}, max_num_seqs=128, max_model_len=1024,
                        kv_cache_gb=2.0, seed=seed, kv_cache_dtype="fp8", **kw)


@pytest.fixture(scope="module")
def run():
    from k8s_llm_monitor_amd import ops
    from k8s_llm_monitor_amd.engine import LLMEngine, SamplingParams

    torch.set_num_threads(16)
    eng = LLMEngine(_cfg(), device="cuda")
    seen, real = [], ops.paged_decode_fused

    def spy(slabs, nslabs, positions, cos_sin, slot_mapping, k_cache, v_cache, *args, **kw):
        seen.append((k_cache.dtype, v_cache.dtype, kw.get("kv_scale") is not None, int(positions.shape[0])))
        return real(slabs, nslabs, positions, cos_sin, slot_mapping, k_cache, v_cache, *args, **kw)

    ops.paged_decode_fused = spy  # what a bucket's graph replays is what its capture launched
    try:
        eng.warmup()
    finally:
        ops.paged_decode_fused = real
    sp = SamplingParams(max_tokens=N_NEW, temperature=0.0, ignore_eos=True)
    seqs3 = eng.generate(_prompts(3, "c"), sp)
    seqs128 = eng.generate(_prompts(128, "a"), sp)
    torch.cuda.synchronize()
    out = {"eng": eng, "seen": seen, "seqs3": seqs3, "seqs128": seqs128, "ref": _fp32_reference(eng.model), "sp": sp}
    yield out
    out.clear()
    del eng
    torch.cuda.empty_cache()


def test_warmup_captures_the_fused_decode_with_an_e4m3_cache(run):
    eng = run["eng"]
    st = eng.stats()
    assert st["kv_cache_dtype"] == "fp8" and eng.runner.k_cache.dtype == F8 and eng.runner.kv_scale is not None
    assert 128 in st["graph_buckets"] and eng.runner.graphs
    assert run["seen"], "warmup never launched paged_decode_fused"
    assert all(kd == F8 and vd == F8 and has_scale for kd, vd, has_scale, _ in run["seen"]), run["seen"][:4]
    assert {rows for *_, rows in run["seen"]} >= {1, 128}
    # the budget holds ~1.94x the blocks of a bf16 cache: codes + scales are the true bytes
    r = eng.runner
    assert st["kv_cache_bytes"] == r.k_cache.numel() + r.v_cache.numel() + 4 * r.kv_scale.numel() <= 2.0 * (1 << 30)
    bf16_blocks = int(2.0 * (1 << 30)) // (2 * 2 * r.model.hkv * 128 * 16 * 2)
    assert st["kv_blocks"] >= 1.9 * bf16_blocks


def _check(run, eng, seqs, which, chunk=None):
    ref = run["ref"]
    for i in which:
        s = seqs[i]
        assert len(s.output_ids) == N_NEW
        p = len(s.prompt_ids)
        ids, rows = s.prompt_ids + s.output_ids, list(range(p - 1, p - 1 + N_NEW))
        lr = _logits(ref, ids, rows, "cpu")
        lg = _logits(eng.model, ids, rows, "cuda")
        scale = float(lr.abs().max())
        err = float((lg - lr).abs().max())
        l8 = _paged_logits(ref, s.prompt_ids, s.output_ids, F8, chunk)
        lu = _paged_logits(ref, s.prompt_ids, s.output_ids, torch.float32, chunk)
        d_kv = float((l8 - lu).abs().max())
        print(f"seq {i}: prefill logits max-abs err {err:.4f}, d_kv {d_kv:.4f}, scale {scale:.3f}")
        assert float((lu - lr).abs().max()) < 1e-3 * scale, "the paged fp32 reference is the plain fp32 reference"
        assert err < 0.03 * scale, f"row {i}: prefill logits max-abs err {err:.4f} vs scale {scale:.3f}"
        assert d_kv > 0, "the fp8 cache changed no logit: the reference is not reading a quantised cache"
        for t in range(N_NEW):
            top, got = float(l8[t].max()), float(l8[t, s.output_ids[t]])
            assert top - got <= 2 * err + 2 * d_kv + 1e-6, (
                f"row {i} step {t}: token {s.output_ids[t]} logit {got:.4f} vs max {top:.4f} "
                f"(bf16 err {err:.4f}, d_kv {d_kv:.4f})")


def test_batch_of_3_matches_the_fp32_model_over_an_fp8_cache(run):
    assert len(run["seqs3"]) == 3
    _check(run, run["eng"], run["seqs3"], range(3))


def test_batch_of_128_matches_the_fp32_model_over_an_fp8_cache(run):
    assert len(run["seqs128"]) == 128 and all(len(s.output_ids) == N_NEW for s in run["seqs128"])
    _check(run, run["eng"], run["seqs128"], CHECKED_128)


def test_prefix_caching_and_chunked_prefill_on_an_fp8_cache(run):
    """A prompt longer than max_prefill_tokens: later chunks attend the earlier ones dequantised
    through the v1 paged prefill's fp8 branch.  The reference prefills in the same chunks."""
    from k8s_llm_monitor_amd.engine import LLMEngine

    eng = LLMEngine(_cfg(seed=5, prefix_caching=True, max_prefill_tokens=48, mixed_prefill_tokens=48), device="cuda")
    eng.model.copy_weights_from(run["eng"].model)
    eng.warmup()
    prompt = " ".join(_prompts(6, "p"))
    seqs = eng.generate([prompt], run["sp"])
    again = eng.generate([prompt], run["sp"])  # its blocks are now prefix-cache hits
    torch.cuda.synchronize()
    assert len(seqs[0].prompt_ids) > 2 * 48
    assert eng.runner.n_steps.get("prefill_context_tokens", 0) > len(seqs[0].prompt_ids)
    _check(run, eng, seqs, [0], chunk=48)
    # the second run attends (almost) the whole prompt dequantised: same rule against the
    # reference with every full prompt block cached
    hit = (len(again[0].prompt_ids) - 1) // 16 * 16
    assert len(again[0].output_ids) == N_NEW
    _check(run, eng, again, [0], chunk=hit)
    del eng
    torch.cuda.empty_cache()

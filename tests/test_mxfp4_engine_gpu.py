"""An engine decoding from MXFP4 weights at Llama-3-8B dimensions (2 layers), graphs on, up to 128
rows per step: tests/test_fp8_engine_gpu.py for the mxfp4 encoding.

The decode graphs must have captured mxfp4 launches of all three epilogues (slabs, LM head, SwiGLU)
in a bucket of at most 32 rows and in the 128-row bucket.  Batches of 3 and of 128 prompts are
checked by the rule of tests/test_decode_batch128_gpu.py against the fp32 CPU model given the
engine's weights through copy_weights_from - the dequantised values, so the reference computes
with exactly the weights the mxfp4 kernels stream: GPU prefill logits within 0.03 x scale, every
greedy token within 2 x err of the fp32 argmax.  A bf16-decoding engine given the same weights must
emit identical tokens (the mxfp4 launches are bit-identical to the bf16 ones)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
N_NEW = 6
CHECKED_128 = [0, 64, 127]


def _fp32_reference(gpu_model):  # as tests/test_decode_batch128_gpu.py
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


def _prompts(n, tag):
    return [f"{tag} node-{i:03d} CPU={30 + i % 60}% pod payments-{i} restarts={i % 7} 为什么我的pod频繁重启？" for i in range(n)]


def _cfg(seed=5, **kw):
    from k8s_llm_monitor_amd.engine import EngineConfig

    return EngineConfig(model="llama-3-8b", model_overrides={"n_layers": 2}, max_num_seqs=128, max_model_len=1024,
                        kv_cache_gb=2.0, seed=seed, prefix_caching=False, **kw)


@pytest.fixture(scope="module")
def run():
    from k8s_llm_monitor_amd import ops
    from k8s_llm_monitor_amd.engine import LLMEngine, SamplingParams

    torch.set_num_threads(16)
    eng = LLMEngine(_cfg(decode_weights="mxfp4"), device="cuda")
    seen, real = [], ops.dec_gemm

    def spy(a, wp, epi, rows, *args, **kw):  # what a bucket's graph replays is what its capture launched
        seen.append((epi, rows, ops.is_mxfp4(wp)))
        return real(a, wp, epi, rows, *args, **kw)

    ops.dec_gemm = spy
    try:
        eng.warmup()
    finally:
        ops.dec_gemm = real
    sp = SamplingParams(max_tokens=N_NEW, temperature=0.0, ignore_eos=True)
    seqs3 = eng.generate(_prompts(3, "c"), sp)
    seqs128 = eng.generate(_prompts(128, "a"), sp)
    torch.cuda.synchronize()
    out = {"eng": eng, "seen": seen, "seqs3": seqs3, "seqs128": seqs128, "ref": _fp32_reference(eng.model), "sp": sp}
    yield out
    out.clear()
    del eng
    torch.cuda.empty_cache()


def test_mxfp4_weights_launched_in_small_and_128_row_buckets(run):
    eng = run["eng"]
    st = eng.stats()
    assert st["decode_weights"] == "mxfp4" and set(st["decode_encodings"].values()) == {"mxfp4"}
    assert 128 in st["graph_buckets"] and eng.runner.graphs
    f4 = {(epi, r) for epi, r, q in run["seen"] if q}
    small = {epi for epi, r in f4 if r <= 32}
    for epi in (0, 1, 2):
        assert epi in small, f"epilogue {epi}: no mxfp4 launch at <= 32 rows: {sorted(f4)}"
        assert (epi, 128) in f4, f"epilogue {epi}: no mxfp4 launch at 128 rows: {sorted(f4)}"
    # resident weights: the bf16 model plus the codes and block scales (17 / 64 of the quantised tensors' bytes)
    m = eng.model
    q_bytes = sum(v.numel() * v.element_size() for L in m.layers for k, v in L.items() if k.endswith(("_q", "_qs")))
    q_bytes += m.lm_head_q.numel() + m.lm_head_qs.numel()
    d_bytes = sum(v.numel() * 2 for L in m.layers for k, v in L.items() if k.endswith("_d")) + m.lm_head_d.numel() * 2
    assert q_bytes * 64 == d_bytes * 17
    assert st["resident_weight_bytes"] == m.resident_weight_bytes() > 3 * q_bytes > 0


def _check_fp32(run, seqs, which):
    for i in which:
        s = seqs[i]
        assert len(s.output_ids) == N_NEW
        p = len(s.prompt_ids)
        ids, rows = s.prompt_ids + s.output_ids, list(range(p - 1, p - 1 + N_NEW))
        lr = _logits(run["ref"], ids, rows, "cpu")
        lg = _logits(run["eng"].model, ids, rows, "cuda")
        scale = float(lr.abs().max())
        err = float((lg - lr).abs().max())
        print(f"seq {i}: prefill logits max-abs err {err:.4f} scale {scale:.3f}")
        assert err < 0.03 * scale, f"row {i}: prefill logits max-abs err {err:.4f} vs scale {scale:.3f}"
        for t in range(N_NEW):
            top, got = float(lr[t].max()), float(lr[t, s.output_ids[t]])
            assert top - got <= 2 * err + 1e-6, (
                f"row {i} step {t}: token {s.output_ids[t]} logit {got:.4f} vs max {top:.4f} (bf16 err {err:.4f})")


def test_batch_of_3_matches_fp32_over_the_dequantised_weights(run):
    assert len(run["seqs3"]) == 3
    _check_fp32(run, run["seqs3"], range(3))


def test_batch_of_128_matches_fp32_over_the_dequantised_weights(run):
    assert len(run["seqs128"]) == 128 and all(len(s.output_ids) == N_NEW for s in run["seqs128"])
    _check_fp32(run, run["seqs128"], CHECKED_128)


def test_bf16_decoding_engine_with_the_same_weights_emits_identical_tokens(run):
    from k8s_llm_monitor_amd.engine import LLMEngine

    eng = LLMEngine(_cfg(seed=6), device="cuda")
    assert set(eng.stats()["decode_encodings"].values()) == {"bf16"}
    eng.model.copy_weights_from(run["eng"].model)
    eng.warmup()
    seqs = eng.generate(_prompts(3, "c"), run["sp"])
    torch.cuda.synchronize()
    assert [s.output_ids for s in seqs] == [s.output_ids for s in run["seqs3"]]
    del eng
    torch.cuda.empty_cache()

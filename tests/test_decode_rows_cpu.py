"""Decode steps of 65..128 rows stay on the skinny path (_decode_layers_skinny over ops.dec_gemm)
for dense TP=1 models: the control flow on the CPU forms of the ops, with CausalLM.DEC_ROWS_MAX as
the A/B switch back to the 64-row routing, and the models that keep the 64-row limit."""
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.models import CausalLM, get_config
from k8s_llm_monitor_amd.parallel.state import ParallelState

ROWS = 96
PROMPTS = [f"pod ns-{i % 7}/svc-{i} restarted {i} times on node-{i % 13:03d}" for i in range(ROWS)]


def _run(monkeypatch, limit):
    """96 prompts, greedy, 4 tokens; returns (tokens, first 96-row decode step's logits, the row
    counts ops.dec_gemm saw)."""
    monkeypatch.setattr(CausalLM, "DEC_ROWS_MAX", limit)
    eng = LLMEngine(EngineConfig(model="llama-tiny-d128", max_num_seqs=ROWS, max_model_len=256, num_blocks=512,
                                 use_graphs=False, seed=3, dtype="float32"), device="cpu")
    assert eng.model.dec_rows_max() == limit
    seen, first = [], []
    real_gemm, real_fwd = ops.dec_gemm, CausalLM.forward

    def spy_gemm(a, wp, epi, rows, *args, **kw):
        seen.append(rows)
        return real_gemm(a, wp, epi, rows, *args, **kw)

    def spy_fwd(self, ids, meta, kv_caches=None):
        out = real_fwd(self, ids, meta, kv_caches)
        if not meta.is_prefill and ids.shape[0] == ROWS and not first:
            first.append(out.detach().float().clone())
        return out

    monkeypatch.setattr(ops, "dec_gemm", spy_gemm)
    monkeypatch.setattr(CausalLM, "forward", spy_fwd)
    seqs = eng.generate(PROMPTS, SamplingParams(max_tokens=4, temperature=0.0, ignore_eos=True))
    assert all(len(s.output_ids) == 4 for s in seqs)
    assert first, "a decode step with all 96 rows ran"
    return [s.output_ids for s in seqs], first[0], seen


def test_decode_96_rows_on_dec_gemm_matches_generic(monkeypatch):
    """With DEC_ROWS_MAX = 128 a 96-row decode step calls ops.dec_gemm with rows == 96 (before, the
    step left the skinny path above 64 rows); with DEC_ROWS_MAX = 64 the same engine and seed take
    the generic layer loop.  The first decode step's logits agree within 1e-4 in fp32 - the bound
    of the CPU skinny-versus-generic comparison
    tests/test_skinny_pack.py::test_decode_skinny_path_matches_generic_cpu."""
    tok_new, lg_new, seen_new = _run(monkeypatch, 128)
    assert ROWS in seen_new
    tok_old, lg_old, seen_old = _run(monkeypatch, 64)
    assert all(r <= 64 for r in seen_old), "the 64-row routing never passes more than 64 rows to dec_gemm"
    assert lg_new.shape == lg_old.shape and lg_new.shape[0] == ROWS
    err = (lg_new - lg_old).abs().max().item()
    print(f"first 96-row decode step: max |logit difference| {err:.3g}")
    assert err < 1e-4


def test_dec_config_up_to_64_rows_is_the_table():
    for (N, K, epi), cfg in ops.DEC_TABLE.items():
        for rows in (0, 1, 33, 64):
            assert ops.dec_config(N, K, epi, rows=rows) == cfg
        assert ops.dec_config(N, K, epi) == cfg
        wide = ops.dec_config(N, K, epi, rows=65)
        assert wide is not None and wide == ops.dec_config(N, K, epi, rows=128)
        assert ops.dec_config(N, K, epi, rows=129) is None
    assert (ops.SKINNY_MAX_M, ops.DEC_MAX_M) == (64, 128)


def test_cpu_dec_gemm_slices_by_the_row_counts_config():
    """The CPU reference of dec_gemm writes as many slabs as the configuration for that row count."""
    N, K, M = 1536, 512, 96
    g = torch.Generator().manual_seed(0)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.05
    cfg = ops.dec_config(N, K, 0, rows=M)
    ws = torch.full((cfg[0] * M * N,), float("nan"))
    assert ops.dec_gemm(ops.pack_activation(x), ops.pack_skinny(w), 0, M, workspace=ws) == cfg[0]
    torch.testing.assert_close(ws.view(cfg[0], M, N).sum(0), x @ w.t(), rtol=1e-4, atol=1e-4)
    with pytest.raises(ValueError):
        ops.dec_gemm(ops.pack_activation(torch.randn(129, K)), ops.pack_skinny(w), 0, 129,
                     workspace=torch.empty(16 * 129 * N))


def test_row_limit_per_model():
    """128 for a dense TP=1 model with every decode copy; 64 for MoE and for a TP=2 shard (the limit
    is decided at construction from the TP degree: no collective runs, so the shard is built in
    this process as the rank-0 half of a 2-rank group)."""
    dense = CausalLM(get_config("llama-tiny-d128"), device="cpu", dtype=torch.float32, seed=1)
    assert dense.dec_rows_max() == 128 == ops.DEC_MAX_M
    assert dense._skinny_ws.numel() % 128 == 0
    moe = CausalLM(get_config("mixtral-tiny"), device="cpu", dtype=torch.float32, seed=1)
    assert moe._skinny_ws is not None and moe.dec_rows_max() == 64
    tp2 = CausalLM(get_config("llama-tiny-d128"), device="cpu", dtype=torch.float32, seed=1,
                   pstate=ParallelState(world_size=2, tp_size=2))
    assert tp2.tp == 2 and tp2._skinny_ws is not None and tp2.dec_rows_max() == 64

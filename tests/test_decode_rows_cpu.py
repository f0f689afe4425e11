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


# ---------------------------------------------------------------- the table of compiled forms

# ops.dec_config's picks for every projection and LM head of Llama-3-8B, Llama-3-70B and
# Mixtral-8x7B at TP 1, 2, 4, 8, recorded before dec_config built its candidates from
# ops.DEC_FORMS: they must not move.
MODELS = {  # d_model, q heads, kv heads (D = 128), ffn, vocab, experts
    "llama-3-8b": (4096, 32, 8, 14336, 128256, 0),
    "llama-3-70b": (8192, 64, 8, 28672, 128256, 0),
    "mixtral-8x7b": (4096, 32, 8, 14336, 32000, 8),
}
DENSE_PINS = {  # (N, K, epi): (pick at 64 rows, pick at 128 rows)
    (768, 4096, 0): ((16, 1, 4, 8), (16, 1, 4, 8)),
    (1280, 8192, 0): ((16, 1, 4, 16), (16, 1, 4, 8)),
    (1536, 4096, 0): ((16, 1, 8, 8), (16, 1, 8, 8)),
    (2560, 8192, 0): ((16, 1, 8, 8), (16, 1, 8, 8)),
    (3072, 4096, 0): ((8, 1, 8, 8), (8, 1, 8, 8)),
    (3584, 4096, 2): ((1, 1, 7, 8), (1, 1, 7, 8)),
    (4032, 4096, 1): ((1, 1, 8, 8), (1, 2, 8, 8)),
    (4096, 512, 0): ((2, 1, 8, 8), (2, 1, 8, 8)),
    (4096, 1024, 0): ((4, 1, 4, 8), (4, 1, 4, 8)),
    (4096, 1792, 0): ((1, 1, 8, 8), (1, 1, 8, 8)),
    (4096, 2048, 0): ((8, 1, 8, 8), (8, 1, 8, 8)),
    (4096, 3584, 0): ((2, 1, 8, 8), (2, 1, 8, 8)),
    (4096, 4096, 0): ((8, 1, 8, 8), (8, 1, 8, 8)),
    (4096, 7168, 0): ((4, 1, 4, 8), (4, 1, 4, 8)),
    (4096, 14336, 0): ((8, 1, 8, 8), (8, 1, 8, 8)),
    (5120, 8192, 0): ((8, 1, 8, 8), (8, 1, 8, 8)),
    (6144, 4096, 0): ((4, 1, 6, 8), (4, 1, 6, 8)),
    (7168, 4096, 2): ((1, 1, 7, 8), (1, 1, 7, 8)),
    (7168, 8192, 2): ((1, 1, 7, 8), (1, 1, 7, 8)),
    (8000, 4096, 1): ((1, 1, 8, 8), (1, 2, 8, 8)),
    (8192, 1024, 0): ((4, 1, 8, 8), (4, 1, 8, 8)),
    (8192, 2048, 0): ((4, 1, 8, 8), (4, 1, 8, 8)),
    (8192, 3584, 0): ((2, 1, 4, 8), (2, 1, 4, 8)),
    (8192, 4096, 0): ((4, 1, 8, 8), (4, 1, 8, 8)),
    (8192, 7168, 0): ((4, 1, 8, 8), (4, 1, 8, 8)),
    (8192, 8192, 0): ((4, 1, 8, 8), (4, 1, 8, 8)),
    (8192, 14336, 0): ((4, 1, 8, 8), (4, 1, 8, 8)),
    (8192, 28672, 0): ((4, 1, 8, 8), (4, 1, 8, 8)),
    (10240, 8192, 0): ((4, 1, 8, 8), (4, 1, 8, 8)),
    (14336, 4096, 2): ((1, 1, 7, 8), (1, 1, 7, 8)),
    (14336, 8192, 2): ((1, 1, 7, 8), (1, 1, 7, 8)),
    (16000, 4096, 1): ((1, 1, 8, 8), (1, 2, 8, 8)),
    (16064, 4096, 1): ((1, 1, 8, 8), (1, 2, 8, 8)),
    (16064, 8192, 1): ((1, 1, 8, 8), (1, 2, 8, 8)),
    (28672, 4096, 2): ((1, 1, 7, 8), (1, 1, 7, 8)),
    (28672, 8192, 2): ((1, 1, 7, 8), (1, 1, 7, 8)),
    (32000, 4096, 1): ((1, 1, 8, 8), (1, 2, 8, 8)),
    (32064, 4096, 1): ((1, 1, 8, 8), (1, 2, 8, 8)),
    (32064, 8192, 1): ((1, 1, 8, 8), (1, 2, 8, 8)),
    (57344, 8192, 2): ((1, 1, 8, 16), (1, 1, 7, 8)),
    (64128, 4096, 1): ((1, 2, 8, 8), (1, 2, 8, 8)),
    (64128, 8192, 1): ((1, 2, 8, 8), (1, 2, 8, 8)),
    (128256, 4096, 1): ((1, 4, 8, 4), (1, 2, 8, 8)),
    (128256, 8192, 1): ((1, 4, 8, 4), (1, 2, 8, 8)),
}
GROUPED_PINS = {  # Mixtral's expert gate_up / down, (N, K, epi, local experts): pick
    (4096, 14336, 0, 1): (8, 1, 8, 8),
    (4096, 14336, 0, 2): (1, 1, 8, 8),
    (4096, 14336, 0, 4): (1, 1, 4, 16),
    (4096, 14336, 0, 8): (1, 1, 8, 8),
    (28672, 4096, 2, 1): (1, 1, 7, 8),
    (28672, 4096, 2, 2): (1, 1, 8, 16),
    (28672, 4096, 2, 4): (1, 1, 8, 16),
    (28672, 4096, 2, 8): (1, 1, 8, 16),
}


def _model_shapes():
    """(dense (N, K, epi), grouped (N, K, epi, local experts)) over MODELS at TP 1, 2, 4, 8."""
    dense, grouped = set(), set()
    for d, hq, hkv, ff, vocab, E in MODELS.values():
        for tp in (1, 2, 4, 8):
            q, kv = hq // tp, max(1, hkv // tp)
            dense |= {((q + 2 * kv) * 128, d, 0), (d, q * 128, 0), (-(-vocab // (64 * tp)) * 64, d, 1)}
            if E:  # experts are sharded by count
                grouped |= {(2 * ff, d, 2, E // tp), (d, ff, 0, E // tp)}
            else:
                dense |= {(2 * ff // tp, d, 2), (d, ff // tp, 0)}
    return dense, grouped


def test_dec_config_picks_pinned():
    dense, grouped = _model_shapes()
    assert dense == set(DENSE_PINS) and grouped == set(GROUPED_PINS)
    for (N, K, epi), picks in DENSE_PINS.items():
        assert (ops.dec_config(N, K, epi, rows=64), ops.dec_config(N, K, epi, rows=128)) == picks, (N, K, epi)
    for (N, K, epi, E), pick in GROUPED_PINS.items():
        assert ops.dec_config(N, K, epi, experts=E) == pick, (N, K, epi, E)
        assert ops.dec_config(N, K, epi, experts=E, rows=64) == pick


def test_every_pick_is_a_compiled_form():
    for (_, _, epi), cfg in ops.DEC_TABLE.items():
        assert ops.dec_form_ok(epi, cfg, 64)
    for (_, _, epi), cfg in ops.DEC_TABLE_M128.items():
        assert ops.dec_form_ok(epi, cfg, 128)
    for (_, _, epi), (c64, c128) in DENSE_PINS.items():
        assert ops.dec_form_ok(epi, c64, 64) and ops.dec_form_ok(epi, c128, 128)
    for (_, _, epi, E), cfg in GROUPED_PINS.items():
        assert ops.dec_form_ok(epi, cfg, 64, grouped=E > 1)


def test_dec_form_ok_refuses_what_is_not_compiled():
    narrow = [f for f in ops.DEC_FORMS if f[4] == 4]
    assert narrow and any(f[4] == 8 for f in ops.DEC_FORMS)
    for epi, ntw, waves, depth, mt, wide in ops.DEC_FORMS:
        cfg = (1, ntw, waves, depth)
        assert ops.dec_form_ok(epi, cfg, 1) and ops.dec_form_ok(epi, cfg, 16 * mt)
        assert ops.dec_form_ok(epi, cfg, 65) == (mt > 4)  # a 4 m-tile form stops at 64 rows
        assert not ops.dec_form_ok(epi, cfg, 129)
        assert ops.dec_form_ok(epi, cfg, 64, grouped=True) and not ops.dec_form_ok(epi, cfg, 65, grouped=True)
        assert ops.dec_form_ok(epi, cfg, 64, wide_norm=True) == bool(wide)
        assert not ops.dec_form_ok(epi, cfg, 65, wide_norm=True)
    assert not ops.dec_form_ok(0, (1, 2, 8, 8), 1)  # (ntw 2, 8 waves, depth 8) is a BF16 form only
    assert any(f[5] for f in ops.DEC_FORMS) and not all(f[5] for f in ops.DEC_FORMS)
    assert ops.dec_row_classes() == (64, 128)
    assert ops.DEC_MAX_M == 128 == ops.dec_row_classes()[-1]
    assert all(any(g[:4] == f for g in ops.DEC_FORMS) for f in ops.DEC_FORMS_TABLE_ONLY)


def test_split_k_workspace_of_the_tiny_model_unchanged():
    """TP=1 dense llama-tiny-d128: the workspace is sized over the row classes, as it was over
    (1, DEC_MAX_M) - 393216 floats."""
    dense = CausalLM(get_config("llama-tiny-d128"), device="cpu", dtype=torch.float32, seed=1)
    assert dense._skinny_ws.numel() == 393216


def test_dec_forms_match_the_extension():
    """ops.DEC_FORMS is the table gemm_decode.hip was compiled from, row for row (no launch)."""
    if not ops.native_available():
        pytest.skip("the extension is not built")
    assert [tuple(r) for r in ops.native().gemm_dec_forms()] == list(ops.DEC_FORMS)

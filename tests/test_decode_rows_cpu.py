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


# ---- dec_plan (csrc/gemm_dec_forms.h) through native().gemm_dec_plan against its Python mirrors

_WF = {None: 0, "fp8": 1, "mxfp4": 2}  # DEC_W_BF16 / DEC_W_F8 / DEC_W_F4


def _plan(enc, M, N, K, S, epi, ntw, waves, depth, f4_depth=0, experts=0, has_row_w=False, rn_nc=0):
    keys = ("err", "mt", "kchunk", "d4", "rnw", "gx", "gy", "gz", "slabs", "max_m")
    return dict(zip(keys, ops.native().gemm_dec_plan(_WF[enc], M, N, K, S, epi, ntw, waves, depth, f4_depth, experts,
                                                      has_row_w, rn_nc)))


def _py_launch_exists(form, enc, E, rows, rn_nc, S, K):
    """The Python side of the same question: ops.dec_form_ok / dec_grouped_q_form_ok, with the
    K-dependent rules dec_config applies before it proposes a configuration (the fp8 K % 64, the
    ``depth`` iteration rule of _dec_pick; mxfp4's whole-256 slices are dec_form_ok's ``K``), the
    launcher's "only slabs split" and "a quantised grouped launch takes no deferred norm"."""
    epi, ntw, waves, depth = form[:4]
    cfg = (S, ntw, waves, depth)
    ksteps = K // 32 // S
    if epi != ops.DEC_SLAB and S != 1:
        return False
    if enc == "fp8" and K % 64:
        return False
    if enc != "mxfp4" and ksteps % max(depth, 8):
        return False
    if E and enc:
        return rn_nc == 0 and ops.dec_grouped_q_form_ok(epi, cfg, rows, K=K, **ops.enc_kw(enc))
    return ops.dec_form_ok(epi, cfg, rows, grouped=E > 0, wide_norm=rn_nc > 16, f8=enc == "fp8", f4=enc == "mxfp4", K=K)


def test_dec_plan_accepts_exactly_what_the_python_rules_accept():
    """Every DEC_FORMS row x weight format x dense / grouped (E 1, 2) x rows x deferred norm (none,
    narrow 4, wide 32 partial sums) x splits (1, 2) at N = 16 ntw waves and 256- and 512-deep K
    slices: the plan's err is 0 exactly where the Python rules say the launch exists; its slab count
    is E * splits for slabs and 1 otherwise; the mxfp4 ring depth follows ops.dec_f4_depth.  No launch."""
    if not ops.native_available():
        pytest.skip("the extension is not built")
    n_ok = 0
    for form in ops.DEC_FORMS:
        epi, ntw, waves, depth = form[:4]
        N = 16 * ntw * waves
        for enc in (None, "fp8", "mxfp4"):
            for E in (0, 1, 2):
                for rows in (1, 16, 17, 64, 65, 128, 129):
                    for rn_nc in (0, 4, 32):
                        for S in (1, 2):
                            for kslice in (256, 512):
                                K = kslice * S
                                for rw in ((False, True) if E and epi == ops.DEC_SLAB else (False,)):
                                    p = _plan(enc, rows, N, K, S, epi, ntw, waves, depth, experts=E, has_row_w=rw,
                                              rn_nc=rn_nc)
                                    want = _py_launch_exists(form, enc, E, rows, rn_nc, S, K)
                                    what = f"{form} {enc} E={E} rows={rows} rn_nc={rn_nc} S={S} K={K} rw={rw}: {p}"
                                    assert (p["err"] == 0) == want, what
                                    assert p["max_m"] == (ops.DEC_NARROW_MAX_M if E else ops.DEC_MAX_M), what
                                    if p["err"]:
                                        continue
                                    n_ok += 1
                                    assert p["slabs"] == (max(E, 1) * S if epi == ops.DEC_SLAB else 1), what
                                    assert (p["mt"], p["kchunk"], p["rnw"]) == (-(-rows // 16), kslice, int(rn_nc > 16)), what
                                    assert (p["gx"], p["gy"], p["gz"]) == (1, S, max(E, 1)), what
                                    if enc != "mxfp4":
                                        assert p["d4"] == 0, what
                                        continue
                                    deep = rows <= 16 and ops.dec_f4_depth(epi, (S, ntw, waves, depth)) == 16 and kslice % 512 == 0
                                    assert p["d4"] == (16 if deep else 8), what
                                    for force in (8, 16):
                                        pf = _plan(enc, rows, N, K, S, epi, ntw, waves, depth, f4_depth=force, experts=E,
                                                   has_row_w=rw, rn_nc=rn_nc)
                                        assert (pf["err"] == 0) == (force == 8 or deep), what
                                        assert pf["err"] or pf["d4"] == force, what
                                    assert _plan(enc, rows, N, K, S, epi, ntw, waves, depth, f4_depth=4, experts=E,
                                                 has_row_w=rw, rn_nc=rn_nc)["err"] == -3, what
    assert n_ok > 1000


@pytest.mark.parametrize("enc", [None, "fp8", "mxfp4"])
def test_dec_plan_refusal_codes(enc):
    """One refusal of each class per weight format, on a SWIGLU8 / SLAB row every format has."""
    if not ops.native_available():
        pytest.skip("the extension is not built")
    assert all(ops.DEC_FORMS[i][:4] in ((0, 1, 8, 8), (2, 1, 7, 8)) for i in (0, 4))
    assert _plan(enc, 64, 128, 512, 2, 0, 1, 8, 8)["err"] == 0
    assert _plan(enc, 129, 128, 512, 2, 0, 1, 8, 8)["err"] == -1  # rows
    assert _plan(enc, 64, 120, 512, 2, 0, 1, 8, 8)["err"] == -1  # N % 16
    assert _plan(enc, 64, 128, 512 + 32, 1, 0, 1, 8, 8)["err"] == (-1 if enc else -3)  # K % 64 / 128; bf16: the slice
    assert _plan(enc, 64, 128, 512, 2, 0, 1, 8, 8, experts=2, has_row_w=True)["err"] == 0
    assert _plan(enc, 64, 112, 256, 1, 2, 1, 7, 8, has_row_w=True)["err"] == -1  # routing weights scale slabs only
    assert _plan(enc, 64, 128, 256, 2, 0, 1, 8, 8)["err"] == -3  # 128-deep slices: half an A chunk
    assert _plan(enc, 64, 112, 512, 2, 2, 1, 7, 8)["err"] == -4  # only slabs split
    assert _plan(enc, 64, 128, 512, 2, 0, 1, 5, 8)["err"] == -5  # no such row
    assert _plan(enc, 65, 112, 256, 1, 2, 1, 7, 16)["err"] == (-3 if enc != "mxfp4" else -5)  # depth 16: 4 m-tiles, no mxfp4


def test_dec_refusals_need_no_launch(monkeypatch):
    """A grouped launch at 65 rows and a wide-norm launch over fp8: the plan refuses, and the wrappers
    raise before the extension's launch is reached (the GPU branch of the wrappers, driven here with
    CPU tensors and a native() that fails the test if it is asked to launch)."""
    if not ops.native_available():
        pytest.skip("the extension is not built")
    N, K, E = 128, 256, 2
    for enc in (None, "fp8", "mxfp4"):
        assert _plan(enc, 65, N, K, 1, 0, 1, 8, 8, experts=E)["err"] < 0
        assert _plan(enc, 64, N, K, 1, 0, 1, 8, 8, experts=E)["err"] == 0
    assert _plan("fp8", 1, 112, K, 1, 2, 1, 7, 8, rn_nc=32)["err"] < 0
    assert _plan(None, 1, 112, K, 1, 2, 1, 7, 8, rn_nc=32)["err"] == 0
    assert _plan("fp8", 1, 112, K, 1, 2, 1, 7, 8, rn_nc=16)["err"] == 0

    class NoLaunch:
        def gemm_dec(self, *a, **k):
            raise AssertionError("the launch was reached")

    monkeypatch.setattr(ops, "_gpu", lambda t: True)
    monkeypatch.setattr(ops, "native", lambda: NoLaunch())
    a65 = ops.pack_activation(torch.zeros(65, K, dtype=torch.bfloat16))
    w = torch.zeros(N, K, dtype=torch.bfloat16)
    ws = torch.empty(E * 65 * N)
    with pytest.raises(RuntimeError, match="not compiled for 65 rows of a grouped launch"):
        ops.dec_gemm_grouped(a65, torch.stack([ops.pack_skinny(w)] * E), 0, 65, workspace=ws, cfg=(1, 1, 8, 8))
    for enc in ("fp8", "mxfp4"):
        _, qp, sp = ops.encode_weight(w, enc)
        with pytest.raises(ValueError, match="at most 64 rows"):
            ops.dec_gemm_grouped_q(a65, torch.stack([qp] * E), torch.stack([sp] * E), 0, 65, workspace=ws, cfg=(1, 1, 8, 8))
    _, qp, sp = ops.encode_weight(torch.zeros(112, K, dtype=torch.bfloat16), "fp8", gate_up8=True)
    a1 = ops.pack_activation(torch.zeros(1, K, dtype=torch.bfloat16))
    out = torch.empty(1, 112 // 64 + 1, 64, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="with the wide deferred norm over fp8 weights"):
        ops.dec_gemm(a1, qp, 2, 1, out=out, cfg=(1, 1, 7, 8), wscale=sp, rownorm=(torch.ones(1, 32), 1e-5))
    with pytest.raises(AssertionError, match="the launch was reached"):  # the narrow norm does launch
        ops.dec_gemm(a1, qp, 2, 1, out=out, cfg=(1, 1, 7, 8), wscale=sp, rownorm=(torch.ones(1, 16), 1e-5))

"""MXFP4 decode weights on the CPU path: the quantiser against a brute-force nearest-grid-point
reference, the packed layouts, the table of mxfp4 forms against the native report, the reference
form of ops.dec_gemm over an mxfp4 weight, and an engine decoding from mxfp4 weights against a
bf16-decoding one given its weights."""
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.models.checkpoint import load_checkpoint, save_checkpoint

GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
MANT = torch.tensor([0, 1, 0, 1, 0, 1, 0, 1])  # the mantissa bit of each grid point's code


def _w(N, K, seed=0, std=0.02):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * std).to(torch.bfloat16)


def _spread(N, K):
    """2^((r + k // 32) % 7 - 3): another scale in every neighbouring row and k-block."""
    return torch.exp2(((torch.arange(N)[:, None] + torch.arange(K)[None, :] // 32) % 7 - 3).float())


def _nibbles(codes):
    return torch.stack((codes & 15, codes >> 4), dim=-1).reshape(codes.shape[0], -1)


def _brute(w):
    """The independent reference: per block of 32 the smallest e with amax <= 6 * 2^e, found by
    stepping; per element the nearest of the 8 grid points by exhaustive distance, a tie going to
    the point with mantissa bit 0.  Returns (nibbles [N, K], e [N, K/32])."""
    N, K = w.shape
    wf = w.double().reshape(N, K // 32, 32)
    amax = wf.abs().amax(-1)
    e = torch.zeros(N, K // 32, dtype=torch.long)
    for i in range(N):
        for j in range(K // 32):
            a, x = amax[i, j].item(), 0
            if a > 0:
                while a > 6 * 2.0 ** x:
                    x += 1
                while a <= 6 * 2.0 ** (x - 1):
                    x -= 1
            e[i, j] = max(-60, min(60, x))
    v = (wf / torch.exp2(e.double())[..., None]).abs().clamp(max=6)
    dist = (v[..., None] - GRID.double()).abs()  # [N, K/32, 32, 8]
    best = dist.amin(-1, keepdim=True)
    cand = dist == best  # one grid point, or two at a tie
    code = torch.where(cand & (MANT == 0), torch.arange(8), torch.full((8,), 99)).amin(-1)
    code = torch.where(code == 99, torch.where(cand, torch.arange(8), torch.full((8,), 99)).amin(-1), code)
    code = code | (torch.signbit(wf).long() << 3)
    return code.reshape(N, K).to(torch.uint8), e


# ------------------------------------------------------------------ the quantiser
@pytest.mark.parametrize("shape", [(48, 256), (16, 1024)])
def test_quantiser_matches_brute_force_and_never_clips(shape):
    N, K = shape
    w = (_w(N, K, seed=1).float() * _spread(N, K)).to(torch.bfloat16)
    codes, scales = ops.quantize_mxfp4(w)
    assert codes.dtype == torch.uint8 and codes.shape == (N, K // 2)
    assert scales.dtype == torch.uint8 and scales.shape == (N, K // 32)
    nib, e = _brute(w)
    assert torch.equal(scales.long() - 127, e), "e = ceil(log2(amax / 6)) per (row, block of 32)"
    assert torch.equal(_nibbles(codes), nib), "nearest grid point, ties to the even mantissa, element 2i in the low nibble"
    # nothing clips: amax / 2^e in (3, 6]
    amax = w.float().abs().reshape(N, K // 32, 32).amax(-1)
    r = amax / torch.exp2(e.float())
    assert torch.all(r > 3) and torch.all(r <= 6), (r.min().item(), r.max().item())
    # |w - dq| <= 2^e < amax / 3 (the grid's widest gap is 2)
    dq = ops.dequantize_mxfp4(codes, scales)
    assert dq.dtype == torch.bfloat16
    dq32 = ops.dequantize_mxfp4(codes, scales, torch.float32)
    assert torch.equal(dq.float(), dq32), "dequantised values equal their bf16 rounding"
    err = (w.float() - dq32).abs().reshape(N, K // 32, 32)
    step = torch.exp2(e.float())[..., None]
    assert torch.all(err <= step) and torch.all(step < amax[..., None] / 3)
    # idempotent: the dequantised values quantise to themselves
    assert torch.equal(ops.dequantize_mxfp4(*ops.quantize_mxfp4(dq)), dq)
    with pytest.raises(ValueError):
        ops.quantize_mxfp4(w[:, :48])


def test_quantiser_ties_zero_block_negative_zero_and_clamps():
    w = torch.zeros(8, 64)
    # row 0, block 0: amax 6 -> e = 0; every midpoint of the grid, both signs
    mids = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    w[0, 0] = 6.0
    w[0, 1:8], w[0, 8:15] = mids, -mids
    w[0, 15] = -0.0
    # row 1: the same scaled by 2^-9 (another e, the same codes)
    w[1, :32] = w[0, :32] * 2.0 ** -9
    # row 2, block 1: a single maximum exactly 6 * 2^5 and one just above 3 * 2^5 elsewhere
    w[2, 40], w[3, 40] = 6.0 * 32, 3.0 * 32 * (1 + 2.0 ** -7)
    # rows 4, 5: beyond both clamp ends
    w[4, 0], w[5, 0] = 2.0 ** -80, 2.0 ** 70
    codes, scales = ops.quantize_mxfp4(w)
    nib = _nibbles(codes)
    # ties to the even mantissa: 0.25 -> 0, 0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4
    even = torch.tensor([0, 2, 2, 4, 4, 6, 6], dtype=torch.uint8)
    for r in (0, 1):
        assert nib[r, 0] == 7 and torch.equal(nib[r, 1:8], even) and torch.equal(nib[r, 8:15], even | 8), nib[r, :16]
        assert nib[r, 15] == 8, "-0 is kept"
    assert scales[0, 0] == 127 and scales[1, 0] == 127 - 9
    assert ops.dequantize_mxfp4(codes, scales, torch.float32)[0, 15].signbit()
    # a block of zeros: scale byte 127, codes 0
    assert scales[0, 1] == 127 and torch.all(codes[0, 16:] == 0)
    assert torch.all(scales[6:] == 127) and torch.all(codes[6:] == 0)
    assert scales[2, 1] == 127 + 5 and nib[2, 40] == 7
    assert scales[3, 1] == 127 + 5 and nib[3, 40] == 5, "just above 3 * 2^e stays at e (3 itself would take e - 1)"
    assert scales[4, 0] == 127 - 60 and scales[5, 0] == 127 + 60, "e clamped to +-60"
    assert nib[4, 0] == 0 and nib[5, 0] == 7
    assert torch.isfinite(ops.dequantize_mxfp4(codes, scales, torch.float32)).all()
    m, s = _brute(w)
    assert torch.equal(nib, m) and torch.equal(scales.long() - 127, s)


def test_quantiser_row_chunks_change_nothing(monkeypatch):
    w = (_w(80, 256, seed=2).float() * _spread(80, 256)).to(torch.bfloat16)
    c, s = ops.quantize_mxfp4(w)
    dq = ops.dequantize_mxfp4(c, s)
    monkeypatch.setattr(ops, "_MXFP4_CHUNK", 7 * 256)
    c2, s2 = ops.quantize_mxfp4(w)
    assert torch.equal(c, c2) and torch.equal(s, s2) and torch.equal(ops.dequantize_mxfp4(c, s), dq)


# ------------------------------------------------------------------ layouts
def test_pack_skinny_f4_round_trip_and_fragment_order():
    N, K = 48, 512
    codes = torch.arange(N * K // 2).reshape(N, K // 2).remainder(251).to(torch.uint8)
    scales = torch.arange(N * K // 32).reshape(N, K // 32).remainder(199).to(torch.uint8)
    cp, sp = ops.pack_skinny_f4(codes, scales)
    assert cp.shape == (N // 16, K // 128, 64, 16) and cp.dtype == torch.uint8 and cp.is_contiguous()
    assert sp.shape == (N // 16, K // 128, 16, 4) and sp.dtype == torch.uint8 and sp.is_contiguous()
    c2, s2 = ops.unpack_skinny_f4(cp, sp)
    assert torch.equal(c2, codes) and torch.equal(s2, scales)
    assert ops.is_mxfp4(cp) and not ops.is_mxfp4(codes) and not ops.is_mxfp4(None)
    assert not ops.is_fp8(cp)
    assert ops.skinny_wdims(cp) == (N, K)
    # lane l's dword s: its 8 elements (4 bytes) of k-step 4g + s, in pack_skinny's fragment order
    el = _nibbles(codes).to(torch.int16)  # pack_skinny over the elements
    ps = ops.pack_skinny(el)  # [N/16, K/32, 64, 8]
    pn = torch.stack((cp & 15, cp >> 4), dim=-1).reshape(N // 16, K // 128, 64, 4, 8).to(torch.int16)
    for g in range(K // 128):
        for s in range(4):
            assert torch.equal(pn[:, g, :, s], ps[:, 4 * g + s])
    # scale dword (j, g, r): row 16 j + r, k-steps 4g .. 4g + 3, the first in the low byte
    for j in range(N // 16):
        for g in range(K // 128):
            assert torch.equal(sp[j, g], scales[16 * j:16 * j + 16, 4 * g:4 * g + 4])
    with pytest.raises(ValueError):
        ops.pack_skinny_f4(codes[:, :96], scales[:, :6])  # K = 192
    with pytest.raises(ValueError):
        ops.pack_skinny_f4(codes, scales[:, :4])


def test_codes_and_scales_follow_interleave_gate_up8():
    F, K = 40, 128
    w13 = (_w(2 * F, K, seed=5).float() * _spread(2 * F, K)).to(torch.bfloat16)
    c, s = ops.quantize_mxfp4(w13)
    ci, si = ops.quantize_mxfp4(ops.interleave_gate_up8(w13))
    assert torch.equal(ci, ops.interleave_gate_up8(c)) and torch.equal(si, ops.interleave_gate_up8(s))


# ------------------------------------------------------------------ forms
def test_f4_forms_mirror_the_native_table():
    assert tuple(tuple(r) for r in ops.native().gemm_dec_f4_forms()) == tuple(ops.DEC_F4_FORMS)
    idx = [i for i, _ in ops.DEC_F4_FORMS]
    assert len(set(idx)) == len(idx) and all(0 <= i < len(ops.DEC_FORMS) for i in idx)
    assert all(d in (8, 16) for _, d in ops.DEC_F4_FORMS)
    assert ops.DEC_TABLE_F4 == {} or all(len(k) == 4 for k in ops.DEC_TABLE_F4)


def test_f4_forms_cover_the_llama_tables():
    for table in (ops.DEC_TABLE, ops.DEC_TABLE_M128):
        for (N, K, epi) in table:
            for r in (1, 64, 65, 128):
                cfg = ops.dec_config(N, K, epi, rows=r)
                routed = ops.DEC_TABLE_F4.get((N, K, epi, 128 if r > 64 else 64), cfg)
                assert ops.dec_form_ok(epi, cfg, r, f4=True, K=K), (N, K, epi, cfg, r)
                assert ops.dec_config(N, K, epi, rows=r, f4=True) == routed
    # mxfp4 forms are dense, narrow-norm launches
    assert not ops.dec_form_ok(ops.DEC_SWIGLU8, (1, 1, 7, 8), 16, wide_norm=True, f4=True)
    assert not ops.dec_form_ok(ops.DEC_SLAB, (1, 1, 8, 8), 16, grouped=True, f4=True)
    assert ops.dec_config(4096, 14336, 0, experts=8, f4=True) is None
    # K must be a multiple of the format's 128-deep group
    assert ops.dec_config(4096, 4096 + 64, 0, f4=True) is None and ops.dec_config(4096, 4096 + 32, 0, f4=True) is None
    # a split-K slice must hold whole 256-deep chunks
    assert ops.dec_form_ok(0, (2, 1, 8, 8), 1, f4=True, K=512) and not ops.dec_form_ok(0, (4, 1, 8, 8), 1, f4=True, K=512)
    # a form outside DEC_F4_FORMS is never an mxfp4 answer
    for N, K, epi in ((32000, 4096, 1), (6144, 4096, 0), (1024, 8192, 0)):
        for r in (1, 128):
            c = ops.dec_config(N, K, epi, rows=r, f4=True)
            assert c is None or ops.dec_form_ok(epi, c, r, f4=True, K=K)
    # every existing answer is unchanged by the new keyword's default
    assert ops.dec_config(4096, 4096, 0, f8=True) == ops.dec_config(4096, 4096, 0, f8=True, f4=False)


# ------------------------------------------------------------------ the CPU reference of dec_gemm
@pytest.mark.parametrize("epi", [ops.DEC_SLAB, ops.DEC_BF16, ops.DEC_SWIGLU8])
@pytest.mark.parametrize("rn", [False, True])
def test_dec_gemm_cpu_mxfp4_equals_bf16_over_dequantised(epi, rn):
    N, K, M = 128, 1024, 19
    w = (_w(N, K, seed=7).float() * _spread(N, K)).to(torch.bfloat16)
    if epi == ops.DEC_SWIGLU8:
        w = ops.interleave_gate_up8(w)
    c, s = ops.quantize_mxfp4(w)
    (cp, sp), wp = ops.pack_skinny_f4(c, s), ops.pack_skinny(ops.dequantize_mxfp4(c, s))
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(11)).to(torch.bfloat16)
    a = ops.pack_activation(x)
    rownorm = ((x.float() ** 2).view(M, K // 512, 512).sum(-1), 1e-5) if rn else None
    form = next(ops.DEC_FORMS[i] for i, _ in ops.DEC_F4_FORMS if ops.DEC_FORMS[i][0] == epi)
    for S in ((1, 2) if epi == ops.DEC_SLAB else (1,)):
        cfg = (S,) + tuple(form[1:4])
        outs = []
        for wgt, kw in ((cp, dict(wscale=sp)), (wp, {})):
            if epi == ops.DEC_SLAB:
                ws = torch.full((S * M * N,), float("nan"))
                assert ops.dec_gemm(a, wgt, epi, M, workspace=ws, rownorm=rownorm, cfg=cfg, **kw) == S
                outs.append(ws)
            elif epi == ops.DEC_BF16:
                y = torch.full((M, N), float("nan"), dtype=torch.bfloat16)
                ops.dec_gemm(a, wgt, epi, M, out=y, rownorm=rownorm, cfg=cfg, **kw)
                outs.append(y)
            else:
                act = torch.full((-(-M // 16), N // 64, 64, 8), float("nan"), dtype=torch.bfloat16)
                ops.dec_gemm(a, wgt, epi, M, out=act, rownorm=rownorm, cfg=cfg, **kw)
                outs.append(ops.unpack_skinny(act)[:M])
        assert not torch.isnan(outs[0]).any()
        assert torch.equal(outs[0], outs[1]), f"epi {epi} S {S} rownorm {rn}"


def test_dec_gemm_mxfp4_needs_its_block_scales():
    c, s = ops.quantize_mxfp4(_w(16, 512))
    cp, sp = ops.pack_skinny_f4(c, s)
    a, out = ops.pack_activation(torch.zeros(1, 512, dtype=torch.bfloat16)), torch.empty(1, 16, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="block scales"):
        ops.dec_gemm(a, cp, ops.DEC_BF16, 1, out=out, cfg=(1, 4, 8, 4))
    with pytest.raises(ValueError, match="block scales"):
        ops.dec_gemm(a, cp, ops.DEC_BF16, 1, out=out, cfg=(1, 4, 8, 4), wscale=s)  # unpacked scales


# ------------------------------------------------------------------ engine
PROMPTS = ["pod crashloop in kube-system", "node-003 NotReady 为什么", "x" * 40]
KEYS = ("wqkv", "wo", "w13", "w2")


def _engine(**kw):
    return LLMEngine(EngineConfig(model="llama-tiny", max_num_seqs=4, max_model_len=256, num_blocks=64,
                                  use_graphs=False, dtype="float32", prefix_caching=False, **kw), device="cpu")
    # (no prefix cache: these tests swap an engine's weights between runs of the same prompts)


def _greedy(eng):
    return [s.output_ids for s in eng.generate(PROMPTS, SamplingParams(max_tokens=8, temperature=0.0, ignore_eos=True))]


def _dq(L, key, dtype):
    return ops.dequantize_mxfp4(*ops.unpack_skinny_f4(L[key + "_q"], L[key + "_qs"]), dtype)


@pytest.fixture(scope="module")
def f4_engine():
    return _engine(decode_weights="mxfp4", seed=3)


def test_engine_mxfp4_is_opt_in_and_reported(f4_engine):
    assert EngineConfig().decode_weights == "bf16"
    with pytest.raises(ValueError):
        _engine(decode_weights="int4")
    with pytest.raises(ValueError):
        _engine(decode_weights="mxfp4", prefill_weights="fp8")
    m = f4_engine.model
    st = f4_engine.stats()
    assert st["decode_weights"] == "mxfp4" and st["resident_weight_bytes"] == m.resident_weight_bytes()
    assert set(st["decode_encodings"].values()) == {"mxfp4"}, st["decode_encodings"]
    assert set(m.decode_encodings().values()) == {"mxfp4"}
    assert set(m.prefill_encodings().values()) == {"bf16"}
    plain = _engine(seed=3)
    assert m.num_local_params() == plain.model.num_local_params()
    # the codes and block scales sit beside the weights: 17 bytes per 32 elements (4.25 bits each)
    L = m.layers[0]
    extra = sum(L[k + "_q"].numel() + L[k + "_qs"].numel() for k in KEYS) * len(m.layers)
    extra += m.lm_head_q.numel() + m.lm_head_qs.numel()
    assert m.resident_weight_bytes() == plain.model.resident_weight_bytes() + extra
    for k in KEYS:
        assert (L[k + "_q"].numel() + L[k + "_qs"].numel()) * 32 == L[k + "_d"].numel() * 17


def test_monitor_config_passes_mxfp4_on():
    from k8s_llm_monitor_amd.monitor.app import engine_config
    from k8s_llm_monitor_amd.monitor.config import from_dict

    assert engine_config(from_dict({"llm": {"decode_weights": "mxfp4"}})).decode_weights == "mxfp4"


def test_engine_bf16_weights_are_the_dequantised_values(f4_engine):
    m = f4_engine.model
    for L in m.layers:
        for key in KEYS:
            assert ops.is_mxfp4(L[key + "_q"])
            dq = _dq(L, key, m.dtype)
            assert torch.equal(ops.unpack_skinny(L[key + "_d"]), dq), key
            canon = m.canonical(L, key)
            want = ops.deinterleave_gate_up8(dq) if key == "w13" else dq
            assert torch.equal(canon, want), key
            assert torch.equal(canon, canon.to(torch.bfloat16).to(canon.dtype)), "bf16-exact values"
    head = m.canonical_head()
    assert torch.equal(head, ops.dequantize_mxfp4(*ops.unpack_skinny_f4(m.lm_head_q, m.lm_head_qs), m.dtype))
    if m.cfg.tie_embeddings:
        assert torch.equal(m.embed, head), "one tensor: the embedding table takes the dequantised values too"


def test_engine_mxfp4_launches_mxfp4_weights(f4_engine, monkeypatch):
    seen = []
    real = ops.dec_gemm

    def spy(a, wp, epi, rows, *args, **kw):
        seen.append((epi, ops.is_mxfp4(wp)))
        return real(a, wp, epi, rows, *args, **kw)

    monkeypatch.setattr(ops, "dec_gemm", spy)
    _greedy(f4_engine)
    assert {e for e, f in seen if f} == {0, 1, 2}, seen[:12]
    assert all(f for _, f in seen), "every decode GEMM of this model has an mxfp4 form"


def test_empty_init_mxfp4_model_quantises_what_it_is_given(f4_engine):
    from k8s_llm_monitor_amd.models import CausalLM
    from k8s_llm_monitor_amd.parallel.state import ParallelState

    src = f4_engine.model
    m = CausalLM(src.cfg, device="cpu", dtype=torch.float32, pstate=ParallelState(), init="empty", dec_weights="mxfp4")
    assert not any(k.endswith("_q") for k in m.layers[0]), "uninitialised storage is not quantised"
    m.copy_weights_from(src)
    for key in KEYS:
        assert torch.equal(m.canonical(m.layers[0], key), src.canonical(src.layers[0], key)), key
        assert ops.is_mxfp4(m.layers[0][key + "_q"])
    assert ops.is_mxfp4(m.lm_head_q)


def test_engine_round_trip_bf16_engine_with_mxfp4_engines_weights(f4_engine, tmp_path):
    toks = _greedy(f4_engine)
    other = _engine(seed=9)  # other weights, bf16 decode
    assert _greedy(other) != toks
    other.model.copy_weights_from(f4_engine.model)
    assert not any(k.endswith("_q") for k in other.model.layers[0])
    assert _greedy(other) == toks, "one model, two encodings: the same greedy tokens"
    # save -> load into an mxfp4 model: requantised from the dequantised values, the same values
    save_checkpoint(f4_engine.model, tmp_path / "ckpt")
    third = _engine(decode_weights="mxfp4", seed=11)
    load_checkpoint(third.model, tmp_path / "ckpt")
    for La, Lb in zip(f4_engine.model.layers, third.model.layers):
        for key in KEYS:
            assert torch.equal(third.model.canonical(Lb, key), f4_engine.model.canonical(La, key)), key
            assert torch.equal(_dq(Lb, key, torch.float32), _dq(La, key, torch.float32)), key
    assert _greedy(third) == toks
    # copy_weights_from INTO an mxfp4 model rebuilds its codes from the new weights
    src = _engine(seed=9)
    third.model.copy_weights_from(src.model)
    L = third.model.layers[0]
    assert torch.equal(ops.unpack_skinny(L["wo_d"]), _dq(L, "wo", third.model.dtype))
    assert not torch.equal(third.model.canonical(L, "wo"), f4_engine.model.canonical(f4_engine.model.layers[0], "wo"))

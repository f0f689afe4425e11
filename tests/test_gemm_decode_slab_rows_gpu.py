"""The SLAB epilogue's row-wide 16-byte stores (ops.DEC_SLAB_ROWS), their write-through form
(DEC_SLAB_WT) and the one-split-per-XCD placement (DEC_XCD_SPLITS) of gemm_decode.hip change no slab
bit: for each of them alone and all three together the slab workspace must be torch.equal to the one
written with every switch off - the whole tensor, a finite sentinel pattern and 1024 elements of
slack past S * M * N included, so a store outside the slabs or a hole inside them fails.

Cases: the four SLAB rows of ops.DEC_FORMS at K = 256 x splits (the depth-16 row: 512 x splits), splits
1, 2, 4, 8 and (8-wave row) 16; rows 1, 16, 17, 63, 64 and, where the row has 8 m-tiles, 65 and 128;
N = 16 waves 2 (the workgroups divide it), 16 (waves + 3) (ragged last workgroup), 16 waves 3 (three
column groups: workgroups x splits is no multiple of 8 below 8 splits - the identity placement) and
16 waves 4 (four column groups: the remap at 2 splits as well);
deferred norm off and on (narrow partial sums, as add_norm_partial's); fp8 and mxfp4 weights on the SLAB
rows of DEC_F8_FORMS / DEC_F4_FORMS; grouped launches of 3 experts at 5 and 64 rows with zeros among the
routing weights, over bf16 and fp8 stacks.  One case per form also holds the summed slabs against the
fp32 product under the bound of tests/test_gemm_decode_gpu.py::test_dec_slabs_match_fp32.  The all-off
workspaces are computed once and shared.  Last, a two-layer decode step at Llama-3-8B dimensions and 64
rows, all switches on against all off: equal residual stream and logits."""
import contextlib
import functools

import pytest
import torch

from k8s_llm_monitor_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
SLACK = 1024
OFF = (0, 0, 0)
SWITCHES = {"rows": (1, 0, 0), "rows_wt": (1, 1, 0), "xcd": (0, 0, 1), "all": (1, 1, 1)}
SLAB_FORMS = [f for f in ops.DEC_FORMS if f[0] == ops.DEC_SLAB]
ROWS = (1, 16, 17, 63, 64)
ROWS_WIDE = (65, 128)


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()
    yield
    for c in (_w, _wq, _x, _ss, _stack, _reference):
        c.cache_clear()


@contextlib.contextmanager
def switches(sw):
    ops.DEC_SLAB_ROWS, ops.DEC_SLAB_WT, ops.DEC_XCD_SPLITS = sw
    try:
        yield
    finally:
        ops.DEC_SLAB_ROWS = ops.DEC_SLAB_WT = ops.DEC_XCD_SPLITS = -1


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


@functools.lru_cache(maxsize=None)
def _w(N, K, seed=0):
    return (torch.randn(N, K, device=DEV, generator=_gen(1000 + N + 7 * K + seed)) * 0.02).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _wq(N, K, enc, seed=0):
    """(packed codes, packed scales) of _w in the encoding."""
    return ops.encode_weight(_w(N, K, seed), enc)[1:]


@functools.lru_cache(maxsize=None)
def _x(M, K, seed=0):
    return torch.randn(M, K, device=DEV, generator=_gen(M * 7919 + K + seed)).to(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _ss(M, K):
    """Narrow deferred-norm sums [M, max(1, K / 512)]: positive, different per row and part."""
    return (torch.rand(M, max(1, K // 512), device=DEV, generator=_gen(M + K)) + 0.25) * (K / 2)


def _sentinel(n):
    return (torch.arange(n + SLACK, device=DEV, dtype=torch.float32) % 251.0) - 125.5


def _dense(M, N, K, cfg, enc, norm):
    """The whole workspace after one dense launch under the switches in force."""
    ws = _sentinel(cfg[0] * M * N)
    w, wscale = (_wq(N, K, enc) if enc else (ops.pack_skinny(_w(N, K)), None))
    s = ops.dec_gemm(ops.pack_activation(_x(M, K)), w, 0, M, workspace=ws, cfg=cfg, wscale=wscale,
                     rownorm=(_ss(M, K), 1e-5) if norm else None)
    assert s == cfg[0]
    return ws


@functools.lru_cache(maxsize=None)
def _stack(E, N, K, enc):
    if enc:
        q = [_wq(N, K, enc, seed=e + 1) for e in range(E)]
        return torch.stack([c for c, _ in q]).contiguous(), torch.stack([s for _, s in q]).contiguous()
    return torch.stack([ops.pack_skinny(_w(N, K, seed=e + 1)) for e in range(E)]).contiguous(), None


def _grouped(M, N, K, cfg, enc, E=3):
    ws = _sentinel(E * cfg[0] * M * N)
    a = torch.stack([ops.pack_activation(_x(M, K, seed=e)) for e in range(E)])
    row_w = torch.rand(M, E, device=DEV, generator=_gen(77 + M)) + 0.25
    row_w[torch.arange(M, device=DEV), torch.arange(M, device=DEV) % E] = 0.0  # row m skips expert m % E
    w, wscale = _stack(E, N, K, enc)
    if enc:
        s = ops.dec_gemm_grouped_q(a, w, wscale, 0, M, workspace=ws, row_w=row_w, cfg=cfg)
    else:
        s = ops.dec_gemm_grouped(a, w, 0, M, workspace=ws, row_w=row_w, cfg=cfg)
    assert s == E * cfg[0]
    return ws


@functools.lru_cache(maxsize=None)
def _reference(kind, *case):
    """The all-off workspace of a case: computed once, shared by the four switch settings."""
    with switches(OFF):
        ref = (_grouped if kind == "grouped" else _dense)(*case)
    n = ref.numel() - SLACK
    assert torch.equal(ref[n:], _sentinel(n)[n:]), f"{kind} {case}: the all-off launch wrote past its slabs"
    assert not torch.equal(ref[:n], _sentinel(n)[:n])
    return ref


def _same(kind, sw, *case):
    with switches(sw):
        got = (_grouped if kind == "grouped" else _dense)(*case)
    ref = _reference(kind, *case)
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero().flatten()
        raise AssertionError(f"{kind} {case} switches {sw}: {bad.numel()} of {ref.numel()} workspace elements differ "
                             f"from the all-off launch, first at {int(bad[0])} (slabs end at {ref.numel() - SLACK})")


def _dense_cases(form):
    _, ntw, waves, depth, max_mt, _ = form
    kstep = 512 if depth == 16 else 256
    for S in (1, 2, 4, 8) + ((16,) if waves == 8 else ()):
        for M in ROWS + (ROWS_WIDE if max_mt == 8 else ()):
            for N in (16 * waves * 2, 16 * (waves + 3), 16 * waves * 3, 16 * waves * 4):
                for norm in (False, True):
                    yield M, N, kstep * S, (S, ntw, waves, depth), None, norm


def _plan(M, N, K, cfg, sw, enc=None, experts=0, rw=False):
    wf = {None: 0, "fp8": 1, "mxfp4": 2}[enc]
    p = ops.native().gemm_dec_plan(wf, M, N, K, cfg[0], 0, *cfg[1:], 0, experts, rw, 0, *sw)
    assert p[0] == 0, (M, N, K, cfg, enc)
    return tuple(p[10:13])


@pytest.mark.parametrize("sw", SWITCHES.values(), ids=SWITCHES.keys())
@pytest.mark.parametrize("form", SLAB_FORMS, ids=lambda f: "w%dd%d" % (f[2], f[3]))
def test_bf16_slabs_bit_equal(form, sw):
    took = set()
    for case in _dense_cases(form):
        M, N, K, cfg = case[:4]
        plan = _plan(M, N, K, cfg, sw)
        assert plan == ops.dec_slab_plan(M, N, cfg, sw=sw)
        gx = -(-(N // 16) // (cfg[1] * cfg[2]))
        rows = int(bool(sw[0]) and M > 16)  # one m-tile keeps the 4-byte stores: the switch changes nothing there
        assert plan == (rows, rows & sw[1], int(bool(sw[2]) and cfg[0] in (2, 4, 8) and gx * cfg[0] % 8 == 0))
        took.add((cfg[0], plan[2]))
        _same("dense", sw, *case)
    if sw[2]:  # both placements were run: the remap at 2, 4 and 8 splits, the identity at 1, 2, 4 (and 16)
        assert {(2, 1), (4, 1), (8, 1), (1, 0), (2, 0), (4, 0)} <= took
        assert form[2] != 8 or (16, 0) in took


@pytest.mark.parametrize("sw", SWITCHES.values(), ids=SWITCHES.keys())
@pytest.mark.parametrize("enc", ["fp8", "mxfp4"])
def test_quantised_slabs_bit_equal(enc, sw):
    forms = ([ops.DEC_FORMS[i] for i in ops.DEC_F8_FORMS] if enc == "fp8" else [ops.DEC_FORMS[i] for i, _ in ops.DEC_F4_FORMS])
    forms = [f for f in forms if f[0] == ops.DEC_SLAB]
    assert forms
    for _, ntw, waves, depth, max_mt, _ in forms:
        for S in (1, 2, 8):
            for M in (1, 17, 64) + ((128,) if max_mt == 8 else ()):
                for N in (16 * waves * 2, 16 * (waves + 3)):
                    for norm in (False, True):
                        _same("dense", sw, M, N, 256 * S, (S, ntw, waves, depth), enc, norm)  # whole 256-deep mxfp4 slices


@pytest.mark.parametrize("sw", SWITCHES.values(), ids=SWITCHES.keys())
@pytest.mark.parametrize("enc", [None, "fp8"], ids=["bf16", "fp8"])
def test_grouped_slabs_bit_equal(enc, sw):
    for M in (5, 64):
        for N in (256, 176):  # two whole 8-wave workgroups; a ragged second one
            for S in (1, 2):
                cfg = (S, 1, 8, 8)
                rows = int(bool(sw[0]) and M > 16)
                assert _plan(M, N, 256 * S, cfg, sw, enc, experts=3, rw=True) == (rows, rows & sw[1], 0)  # grouped: never remapped
                _same("grouped", sw, M, N, 256 * S, cfg, enc)


@pytest.mark.parametrize("form", SLAB_FORMS, ids=lambda f: "w%dd%d" % (f[2], f[3]))
def test_summed_slabs_match_fp32(form):
    _, ntw, waves, depth, _, _ = form
    M, S, N = 64, 4, 16 * (waves + 3)
    K = (512 if depth == 16 else 256) * S
    with switches((1, 1, 1)):
        ws = _dense(M, N, K, (S, ntw, waves, depth), None, False)
    y = ws[: S * M * N].view(S, M, N).sum(0)
    ref = _x(M, K).float() @ _w(N, K).float().t()
    err, scale = (y - ref).abs().max().item(), ref.abs().max().item()
    assert err <= 2.5e-2 * scale + 1e-3, f"form {form}: max err {err:.4g} vs scale {scale:.4g}"


def test_decode_step_8b_dimensions():
    """64 rows through two Llama-3-8B layers' decode path (qkv on the 6-wave row at 4 splits, o and
    down on the 8-wave row at 8, all three remapped): residual stream and logits, on against off."""
    from k8s_llm_monitor_amd.models import AttnMeta, CausalLM, get_config

    cfg = get_config("llama-3-8b").replace(n_layers=2)
    m = CausalLM(cfg, device=DEV, seed=3)
    assert m._skinny_ws is not None
    B, bs = 64, 16
    lens = (torch.arange(B, dtype=torch.int32, device=DEV) * 5) % 30 + 1
    bt = torch.arange(B * 2, dtype=torch.int32, device=DEV).view(B, 2)
    k, v = ops.kv_cache_alloc(cfg.n_layers, 2 * B, m.hkv, m.D, torch.bfloat16, DEV)
    k.normal_(generator=_gen(1))
    v.normal_(generator=_gen(2))
    ids = torch.randint(0, cfg.vocab_size, (B,), dtype=torch.int32, device=DEV, generator=_gen(3))
    pos = (lens - 1).long()
    slots = (bt[torch.arange(B, device=DEV), pos // bs] * bs + (pos % bs).int()).to(torch.int32)
    meta = AttnMeta(is_prefill=False, positions=lens - 1, slot_mapping=slots, block_tables=bt, seq_lens=lens,
                    decode_ws=ops.decode_workspace(B, m.hq, m.D, device=DEV, Hkv=m.hkv))
    seen, real = [], ops.dec_gemm

    def spy(a, wp, epi, rows, *args, **kw):
        if epi == ops.DEC_SLAB:
            N, K = ops.skinny_wdims(wp)
            seen.append(ops.dec_slab_plan(rows, N, ops.dec_config(N, K, epi, rows=rows)))
        return real(a, wp, epi, rows, *args, **kw)

    out = {}
    for sw in ((1, 1, 1), OFF):
        with switches(sw), torch.no_grad():
            residual = m.embed_tokens(ids)
            ops.dec_gemm = spy
            try:
                logits = m._decode_layers_skinny(None, residual, meta, [(k[i], v[i]) for i in range(cfg.n_layers)])
            finally:
                ops.dec_gemm = real
            out[sw] = (residual.clone(), logits.clone())
    torch.cuda.synchronize()
    # qkv, o, down of two layers, each way, and nothing else
    assert seen.count((1, 1, 1)) == seen.count(OFF) >= 6 and set(seen) == {(1, 1, 1), OFF}, seen
    (ra, la), (rb, lb) = out[(1, 1, 1)], out[OFF]
    assert la.shape == (B, cfg.vocab_size) and torch.isfinite(la.float()).all() and la.float().abs().sum() > 0
    assert torch.equal(ra, rb), "residual stream differs"
    assert torch.equal(la, lb), "logits differ"
    del m
    torch.cuda.empty_cache()

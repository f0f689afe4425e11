"""LoRA adapters on gate_proj / up_proj on the CPU: the opt-in gate_up arena ("w13"), whose delta
enters before SwiGLU.  Model and engine in fp32 against the merged model W + s B A (the oracle and
the tolerance of tests/test_lora_cpu.py), the adapter files with gate / up tensors, the refusals, and
the CPU forms of ops.dec_gemm's pre-activation delta and of the per-16 silu_mul pairing."""
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.models.checkpoint import LoraAdapter, load_lora, merge_lora, save_lora
from k8s_llm_monitor_amd.models.config import get_config
from k8s_llm_monitor_amd.models.llama import CANONICAL, INTERLEAVED, PACKED, AttnMeta, CausalLM
from k8s_llm_monitor_amd.models.reference import fp32_logits

ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")
ALL7 = ATTN + ("down_proj", "gate_proj", "up_proj")
# tests/test_lora_cpu.py MERGED_REL_BOUND: the adapter path against the merged model, both fp32
# (summation order only), measured 1.009e-6 of the logit scale there; the bound is 4 x that
MERGED_REL_BOUND = 4 * 1.009e-6


def _shapes(c):
    D, d = c.head_dim, c.d_model
    return {"q_proj": (c.n_heads * D, d), "k_proj": (c.n_kv_heads * D, d), "v_proj": (c.n_kv_heads * D, d),
            "o_proj": (d, c.n_heads * D), "down_proj": (d, c.ffn_dim), "gate_proj": (c.ffn_dim, d),
            "up_proj": (c.ffn_dim, d)}


def _adapter(c, r, targets, seed, scale=0.1, alpha=None, rslora=False, name=""):
    g = torch.Generator().manual_seed(seed)
    t = {}
    for layer in range(c.n_layers):
        for m in targets:
            out, inn = _shapes(c)[m]
            t[(layer, m)] = (torch.randn(r, inn, generator=g) * scale, torch.randn(out, r, generator=g) * scale)
    return LoraAdapter(r=r, lora_alpha=float(alpha if alpha is not None else 2 * r), target_modules=tuple(sorted(targets)),
                       tensors=t, use_rslora=rslora, name=name)


def _prefill_logits(model, ids, slot=None):
    n = len(ids)
    meta = AttnMeta(is_prefill=True, positions=torch.arange(n, dtype=torch.int32),
                    slot_mapping=torch.full((n,), -1, dtype=torch.int32),
                    cu_seqlens=torch.tensor([0, n], dtype=torch.int32))
    if slot is not None:
        meta.lora_slot = torch.full((n,), slot, dtype=torch.int32)
    return model.forward(torch.tensor(ids, dtype=torch.int32), meta, None).float()


IDS = [1, 17, 33, 250, 5, 99, 140, 7, 61, 200, 3, 45, 300, 12, 90, 41, 8, 77]


# ------------------------------------------------------------------ 1. the model against the merged model

@pytest.mark.parametrize("targets", [ALL7, ("gate_proj",), ("up_proj",), ("gate_proj", "up_proj")])
def test_model_prefill_matches_merged_model(targets):
    c = get_config("llama-tiny")
    ad = _adapter(c, 4, targets, 31, rslora=len(targets) == 2)
    base = CausalLM(c, device="cpu", dtype=torch.float32, seed=11)
    st = base.enable_lora(2, 16, mlp=True)
    assert st.dims["w13"] == (2 * c.ffn_dim, c.d_model, 64)
    base.load_adapter(1, ad)
    merged = CausalLM(c, device="cpu", dtype=torch.float32, seed=11)
    merge_lora(merged, ad)
    ref = _prefill_logits(merged, IDS)
    ours, plain = _prefill_logits(base, IDS, slot=1), _prefill_logits(base, IDS)
    scale = ref.abs().max().item()
    rel = (ours - ref).abs().max().item() / scale
    sep = (plain - ref).abs().max().item() / scale
    print(f"{targets}: adapter path vs merged: {rel:.3e} of the logit scale; base vs merged {sep:.3e}")
    assert rel <= MERGED_REL_BOUND
    assert sep > 1e3 * MERGED_REL_BOUND  # the adapter is no no-op
    # slot 0 holds nothing: its rows are the base model's
    assert torch.equal(_prefill_logits(base, IDS, slot=0), plain)


def test_merge_lora_folds_gate_and_up_into_their_rows():
    c = get_config("llama-tiny")
    F = c.ffn_dim
    for t, lo in (("gate_proj", 0), ("up_proj", F)):
        ad = _adapter(c, 4, (t,), 5)
        m0 = CausalLM(c, device="cpu", dtype=torch.float32, seed=3)
        m1 = CausalLM(c, device="cpu", dtype=torch.float32, seed=3)
        merge_lora(m1, ad)
        for layer in range(c.n_layers):
            w0, w1 = m0.canonical(m0.layers[layer], "w13"), m1.canonical(m1.layers[layer], "w13")
            A, B = ad.tensors[(layer, t)]
            want = w0.double().clone()
            want[lo:lo + F] += ad.scaling * (B.double() @ A.double())
            # merged in fp32: the r-term product, the scaling, the sum and the store each round once
            mag = w0.double().abs()
            mag[lo:lo + F] += (ad.r + 2) * abs(ad.scaling) * (B.double().abs() @ A.double().abs())
            assert bool(((w1.double() - want).abs() <= 2.0 ** -23 * mag).all())
            other = slice(F, 2 * F) if lo == 0 else slice(0, F)
            assert torch.equal(w1[other], w0[other])
            for k in ("wqkv", "wo", "w2"):
                assert torch.equal(m1.canonical(m1.layers[layer], k), m0.canonical(m0.layers[layer], k))


def test_arena_rows_follow_the_resident_layout(monkeypatch):
    """B's rows are stored in the row order of the resident w13, and follow it when a rebuild
    (_init_skinny) changes the layout: a loaded adapter never meets a stale pairing."""
    c = get_config("llama-tiny")
    m = CausalLM(c, device="cpu", dtype=torch.float32, seed=11)
    m.enable_lora(1, 8, mlp=True)
    ad = _adapter(c, 4, ("gate_proj", "up_proj"), 9)
    m.load_adapter(0, ad)
    cap = 32
    canon = torch.zeros(2 * c.ffn_dim, 2 * cap)
    canon[:c.ffn_dim, :4] = ad.tensors[(0, "gate_proj")][1]
    canon[c.ffn_dim:, cap:cap + 4] = ad.tensors[(0, "up_proj")][1]
    fwd = {PACKED: ops.interleave_gate_up8, INTERLEAVED: ops.interleave_gate_up, CANONICAL: lambda w: w}
    first = m._layout
    assert first in fwd and m._lora_w13_layout == first
    assert torch.equal(m.lora.B["w13"][0, 0], fwd[first](canon))
    A = m.lora.A["w13"][0, 0]
    assert torch.equal(A[:4], ad.tensors[(0, "gate_proj")][0]) and torch.equal(A[cap:cap + 4], ad.tensors[(0, "up_proj")][0])
    assert not A[4:cap].any() and not A[cap + 4:].any()
    ref = _prefill_logits(m, IDS, slot=0)
    monkeypatch.setattr(CausalLM, "ONE_LAYOUT", "force")  # the packed tensors become the only copy
    m._init_skinny()
    assert m._layout == PACKED != first and m._lora_w13_layout == PACKED
    assert torch.equal(m.lora.B["w13"][0, 0], ops.interleave_gate_up8(canon))
    got = _prefill_logits(m, IDS, slot=0)
    assert (got - ref).abs().max().item() <= MERGED_REL_BOUND * ref.abs().max().item()
    monkeypatch.setattr(CausalLM, "ONE_LAYOUT", False)
    m._init_skinny()
    assert m._layout == first and torch.equal(m.lora.B["w13"][0, 0], fwd[first](canon))


# ------------------------------------------------------------------ 2. adapter files

def test_save_load_round_trip_with_gate_up(tmp_path):
    c = get_config("llama-tiny")
    a = _adapter(c, 4, ALL7, 1, rslora=True, alpha=12, name="a")
    b = load_lora(save_lora(a, tmp_path / "a"))
    assert (b.r, b.lora_alpha, b.use_rslora, b.target_modules, b.name) == (4, 12.0, True, tuple(sorted(ALL7)), "a")
    assert set(b.tensors) == set(a.tensors) and (0, "gate_proj") in b.tensors and (1, "up_proj") in b.tensors
    for k, (A, B) in a.tensors.items():
        assert torch.equal(b.tensors[k][0], A) and torch.equal(b.tensors[k][1], B)


# ------------------------------------------------------------------ 3. the engine

PROMPTS = ([7 + (5 * i) % 300 for i in range(23)], [11 + (7 * i) % 290 for i in range(20)],
           [3 + (11 * i) % 310 for i in range(27)])
STEPS = 8


@pytest.fixture(scope="module")
def adapter_dirs(tmp_path_factory):
    c = get_config("llama-tiny")
    root = tmp_path_factory.mktemp("adapters")
    a = _adapter(c, 4, ALL7, 21, name="a")
    b = _adapter(c, 8, ("gate_proj", "v_proj"), 22, rslora=True, name="b")
    at = _adapter(c, 4, ATTN, 23, name="attn")
    return {"a": str(save_lora(a, root / "a")), "b": str(save_lora(b, root / "b")),
            "attn": str(save_lora(at, root / "attn"))}


def _engine(adapters=None, **kw):
    cfg = dict(model="llama-tiny", dtype="float32", max_num_seqs=8, max_model_len=256, num_blocks=64, use_graphs=False,
               seed=5, lora_adapters=adapters or {})
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg), device="cpu")


def _run(eng, reqs):
    seqs = [eng.add_request(list(p), SamplingParams(max_tokens=STEPS, temperature=0.0, ignore_eos=True, adapter=ad))
            for p, ad in reqs]
    while eng.has_work():
        eng.step()
    return seqs


@pytest.mark.parametrize("layout", [INTERLEAVED, PACKED])
def test_engine_mixed_batch_matches_merged_engines(adapter_dirs, layout, monkeypatch):
    """INTERLEAVED (the CPU's default: adapter steps take the generic layer loop) and PACKED (the
    skinny decode loop: ops.lora_slab into the workspace, then ops.dec_gemm with the delta)."""
    if layout == PACKED:
        monkeypatch.setattr(CausalLM, "ONE_LAYOUT", "force")
    dirs = {k: adapter_dirs[k] for k in ("a", "b")}
    eng = _engine(dirs)
    st = eng.stats()
    assert eng.model._layout == layout and "w13" in eng.model.lora.dims
    assert st["lora_bytes"] == eng.model.lora.nbytes
    w13 = sum(t[:].numel() * t.element_size() for t in (eng.model.lora.A["w13"], eng.model.lora.B["w13"]))
    assert w13 > 0 and st["lora_bytes"] > w13
    assert st["lora_adapters"] == [{"name": "a", "rank": 4, "targets": sorted(ALL7)},
                                   {"name": "b", "rank": 8, "targets": ["gate_proj", "v_proj"]}]
    with_delta, real = [], ops.dec_gemm
    monkeypatch.setattr(ops, "dec_gemm", lambda *a, **k: (with_delta.append(k.get("delta") is not None), real(*a, **k))[1])
    mixed = [s.output_ids for s in _run(eng, list(zip(PROMPTS, ("a", "b", None))))]
    monkeypatch.setattr(ops, "dec_gemm", real)
    assert any(with_delta) == (layout == PACKED)  # which decode path the adapter steps took
    oracle = []
    for i, name in enumerate(("a", "b", None)):
        m = _engine()
        if name is not None:
            merge_lora(m.model, load_lora(dirs[name]))
        toks = _run(m, [(PROMPTS[i], None)])[0].output_ids
        for j in range(STEPS):  # on the merged model alone: the top-2 margin is far above summation order
            lg = fp32_logits(m.model, torch.tensor(PROMPTS[i] + toks[:j]))[0]
            top = lg.topk(2).values
            assert int(lg.argmax()) == toks[j]
            assert (top[0] - top[1]).item() > 100 * MERGED_REL_BOUND * lg.abs().max().item(), (name, j)
        oracle.append(toks)
    assert mixed == oracle
    base = [_run(_engine(), [(PROMPTS[i], None)])[0].output_ids for i in (0, 1)]
    assert base[0] != oracle[0] and base[1] != oracle[1], "the adapters must change the tokens"


def test_engine_allocates_the_gate_up_arena_only_when_targeted(adapter_dirs):
    eng = _engine({"attn": adapter_dirs["attn"]})
    assert "w13" not in eng.model.lora.dims
    plain = CausalLM(get_config("llama-tiny"), device="cpu", dtype=torch.float32)
    assert eng.stats()["lora_bytes"] == plain.enable_lora(1, eng.cfg.lora_max_rank).nbytes


# ------------------------------------------------------------------ 4. refusals

def test_refusals():
    c = get_config("llama-tiny")
    moe = CausalLM(get_config("mixtral-tiny"), device="cpu", dtype=torch.float32)
    with pytest.raises(ValueError, match="MoE"):
        moe.enable_lora(1, 8, mlp=True)
    m = CausalLM(c, device="cpu", dtype=torch.float32)
    m.enable_lora(1, 8, mlp=False)
    for t in ("gate_proj", "up_proj"):
        with pytest.raises(ValueError, match=r"SwiGLU.*mlp=True"):
            m.load_adapter(0, _adapter(c, 4, (t,), 1))
    assert ops.LORA_PROJ[-1] == "w13"
    ops.LoraState(1, 1, {"w13": (64, 64, ops.LORA_MAX_CAP)}, "cpu", torch.float32)
    with pytest.raises(ValueError, match="exceeds"):
        ops.LoraState(1, 1, {"w13": (64, 64, ops.LORA_MAX_CAP + 1)}, "cpu", torch.float32)
    with pytest.raises(ValueError, match="exceeds"):  # 2 x 128 rank rows
        CausalLM(c, device="cpu", dtype=torch.float32).enable_lora(1, 128, mlp=True)
    CausalLM(c, device="cpu", dtype=torch.float32).enable_lora(1, 64, mlp=True)  # 2 x 64 <= LORA_MAX_CAP


# ------------------------------------------------------------------ 5. the ops' CPU forms

@pytest.mark.parametrize("norm", [False, True])
def test_dec_gemm_cpu_delta_matches_the_formula(norm):
    F, K, M, nslots = 32, 64, 5, 3
    g = torch.Generator().manual_seed(8)
    w = torch.randn(2 * F, K, generator=g) * 0.2  # canonical [gate; up]
    x = torch.randn(M, K, generator=g)
    delta = torch.randn(M, 2 * F, generator=g)  # packed order
    slot = torch.tensor([-1, 0, 2, nslots, 1], dtype=torch.int32)
    wp = ops.pack_skinny(ops.interleave_gate_up8(w))
    rn = None
    sc = torch.ones(M, 1, dtype=torch.float64)
    if norm:
        ss = torch.rand(M, 1, generator=g) * K + 1.0
        rn = (ss, 1e-5)
        sc = torch.rsqrt(ss.double() / K + 1e-5)
    out = ops.packed_empty(M, F, torch.float32, "cpu")
    ops.dec_gemm(ops.pack_activation(x), wp, 2, M, out=out, rownorm=rn, cfg=(1, 1, 7, 8), delta=delta, delta_slot=slot,
                 delta_slots=nslots)
    out0 = ops.packed_empty(M, F, torch.float32, "cpu")
    ops.dec_gemm(ops.pack_activation(x), wp, 2, M, out=out0, rownorm=rn, cfg=(1, 1, 7, 8))
    on = (slot >= 0) & (slot < nslots)
    pre = (x.double() @ ops.interleave_gate_up8(w).double().t()) * sc
    pre[on] += delta.double()[on]
    gu = ops.deinterleave_gate_up8(pre.t()).t()
    want = torch.nn.functional.silu(gu[:, :F]) * gu[:, F:]
    got, got0 = ops._cpu_a(out, M).double(), ops._cpu_a(out0, M).double()
    assert bool(((got - want).abs() <= 1e-5 * (1 + want.abs())).all())
    assert torch.equal(got[~on], got0[~on]) and not torch.equal(got[on], got0[on])
    with pytest.raises(ValueError, match="SwiGLU"):
        ops.dec_gemm(ops.pack_activation(x), wp, 0, M, workspace=torch.zeros(M * 2 * F), cfg=(1, 1, 8, 8), delta=delta,
                     delta_slot=slot, delta_slots=nslots)


def test_silu_mul_pairing8_cpu():
    g = torch.Generator().manual_seed(2)
    F = 24
    gu = torch.randn(3, 2 * F, generator=g)  # [F gate | F up]
    gu[0, 1] = -95.0
    x8 = ops.interleave_gate_up8(gu.t().contiguous()).t().contiguous()
    assert torch.equal(ops.silu_mul(x8, pairing=8), ops.silu_mul(gu))
    assert torch.equal(ops.silu_mul(x8, pairing=8), ops.silu_mul(gu, pairing=0))
    with pytest.raises(ValueError, match="pairing"):
        ops.silu_mul(gu, pairing=4)

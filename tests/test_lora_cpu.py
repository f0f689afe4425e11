"""Per-request LoRA adapters on the CPU: the ops' fp32 forms, the PEFT adapter files, the engine and
the public interface.  The oracle everywhere is the merged model: an adapter applied at run time
must equal the base model whose weights are W + s B A."""
import json

import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.models.checkpoint import (LoraAdapter, load_checkpoint, load_lora, merge_lora, save_checkpoint,
                                                   save_lora)
from k8s_llm_monitor_amd.models.config import get_config
from k8s_llm_monitor_amd.models.llama import AttnMeta, CausalLM
from k8s_llm_monitor_amd.models.reference import fp32_logits

ATTN = ("q_proj", "k_proj", "v_proj", "o_proj")
ALL = ATTN + ("down_proj",)
# test_adapter_files_match_merged_transformers_model: measured max |logit diff| / max |logit| of the
# adapter path against the merged transformers model, both fp32 (summation order only): 1.009e-6
# (alpha / r, all five targets) and 8.76e-7 (rslora, q and v); the bound is 4 x the larger
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


# ------------------------------------------------------------------ 1. the ops' CPU forms

def _arena(N=48, K=64, dtype=torch.bfloat16):
    st = ops.LoraState(3, 1, {"wo": (N, K, 16)}, "cpu", dtype)
    g = torch.Generator().manual_seed(3)
    for s, r in enumerate((1, 5, 16)):
        st.load(s, 0, "wo", torch.randn(r, K, generator=g) * 0.2, torch.randn(N, r, generator=g) * 0.2)
        st.set_scaling(s, (2.0, 0.5, 0.25)[s])
    return st


def _dense(st, x, slot):
    """x @ (s B A)^T in fp64 per row, and the same over absolute values (the error bound's scale)."""
    A, B, sc = st.A["wo"][0].double(), st.B["wo"][0].double(), st.scaling.double()
    W = sc[:, None, None] * (B @ A)  # [slots, N, K]
    Wa = sc.abs()[:, None, None] * (B.abs() @ A.abs())
    d = torch.zeros(x.shape[0], W.shape[1], dtype=torch.float64)
    mag = torch.zeros_like(d)
    for i, s in enumerate(slot.tolist()):
        if s >= 0:
            d[i], mag[i] = W[s] @ x[i].double(), Wa[s] @ x[i].double().abs()
    return d, mag


@pytest.mark.parametrize("packed", [False, True])
def test_lora_ops_cpu_match_the_dense_product(packed):
    N, K, M, R = 48, 64, 19, 32
    st = _arena(N, K)
    x = torch.randn(M, K, generator=torch.Generator().manual_seed(4)).to(torch.bfloat16)
    slot = torch.tensor([(-1, 0, 1, 2)[i % 4] for i in range(M)], dtype=torch.int32)
    d, mag = _dense(st, x, slot)
    bound = (K + R + 8) * 2.0 ** -24 * mag
    ns = 2
    ws = torch.full(((ns + 2) * M * N,), 7.5)
    a = ops.pack_activation(x) if packed else x
    assert ops.lora_slab(st, 0, "wo", a, M, ws, ns, slot) == ns + 1
    got = ws[ns * M * N:(ns + 1) * M * N].view(M, N)
    assert bool((ws[:ns * M * N] == 7.5).all()) and bool((ws[(ns + 1) * M * N:] == 7.5).all())
    assert bool(((got.double() - d).abs() <= bound).all())
    off = slot < 0
    assert torch.equal(got[off], torch.zeros_like(got[off]))
    # the deferred norm scales the rows of the slab
    ss = torch.rand(M, 1, generator=torch.Generator().manual_seed(5)) * K + 1.0
    ws2 = torch.zeros((ns + 1) * M * N)
    ops.lora_slab(st, 0, "wo", a, M, ws2, ns, slot, rownorm=(ss, 1e-5))
    sc = torch.rsqrt(ss.double().sum(1, keepdim=True) / K + 1e-5)
    got2 = ws2[ns * M * N:].view(M, N)
    assert bool(((got2.double() - d * sc).abs() <= bound * sc + 1e-7 * (d * sc).abs()).all())
    # in-place add: rows without an adapter bit-unchanged, the others one rounding of y + delta
    y = (torch.randn(M, N, generator=torch.Generator().manual_seed(6)) * 0.5).to(torch.bfloat16)
    y0 = y.clone()
    ops.lora_add(st, 0, "wo", x, y, slot)
    assert torch.equal(y[off], y0[off])
    tgt = y0.double() + d
    assert bool(((y.double() - tgt).abs()[~off] <= (2.0 ** -8 * tgt.abs() + bound)[~off]).all())
    # a row's result does not depend on the other rows' slots
    slot_b = slot.clone()
    slot_b[1:] = torch.tensor([(2, -1, 0, 1)[i % 4] for i in range(M - 1)], dtype=torch.int32)
    slot_b[5] = slot[5]
    ws3 = torch.zeros((ns + 1) * M * N)
    ops.lora_slab(st, 0, "wo", a, M, ws3, ns, slot_b)
    got3 = ws3[ns * M * N:].view(M, N)
    yb = y0.clone()
    ops.lora_add(st, 0, "wo", x, yb, slot_b)
    for row in (0, 5):
        assert int(slot_b[row]) == int(slot[row])
        assert torch.equal(got3[row], got[row]) and torch.equal(yb[row], y[row])


# ------------------------------------------------------------------ 2. adapter files

def test_lora_save_load_round_trip(tmp_path):
    c = get_config("llama-tiny")
    a = _adapter(c, 4, ALL, 1, rslora=True, alpha=12, name="a")
    b = load_lora(save_lora(a, tmp_path / "a"))
    assert (b.r, b.lora_alpha, b.use_rslora, b.target_modules, b.name) == (4, 12.0, True, tuple(sorted(ALL)), "a")
    assert b.scaling == 12 / 2.0 and _adapter(c, 4, ATTN, 1, alpha=12).scaling == 3.0
    assert set(b.tensors) == set(a.tensors)
    for k, (A, B) in a.tensors.items():
        assert torch.equal(b.tensors[k][0], A) and torch.equal(b.tensors[k][1], B)


def _write_peft_dir(path, c, r, alpha, targets, rslora, seed, cfg_extra=None, extra_tensors=None):
    """A PEFT adapter directory written by hand with the Hugging Face tensor names."""
    from safetensors.torch import save_file

    path.mkdir(parents=True, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for i in range(c.n_layers):
        for m in targets:
            out, inn = _shapes(c)[m]
            parent = "self_attn" if m in ATTN else "mlp"
            sd[f"base_model.model.model.layers.{i}.{parent}.{m}.lora_A.weight"] = torch.randn(r, inn, generator=g) * 0.1
            sd[f"base_model.model.model.layers.{i}.{parent}.{m}.lora_B.weight"] = torch.randn(out, r, generator=g) * 0.1
    sd.update(extra_tensors or {})
    save_file(sd, str(path / "adapter_model.safetensors"), metadata={"format": "pt"})
    cfg = {"peft_type": "LORA", "r": r, "lora_alpha": alpha, "target_modules": list(targets), "use_rslora": rslora,
           "bias": "none", "use_dora": False, "modules_to_save": None}
    cfg.update(cfg_extra or {})
    (path / "adapter_config.json").write_text(json.dumps(cfg))
    return sd


@pytest.mark.parametrize("kind", ["alpha_over_r", "rslora"])
def test_adapter_files_match_merged_transformers_model(tmp_path, kind):
    """A hand-written PEFT directory applied at run time to float32 llama-tiny against a transformers
    LlamaForCausalLM holding the merged weights W + s B A (merged here in fp64 from the file's
    tensors, by name: q, k and v into their own projections; s = alpha / r, or alpha / sqrt(r) with
    rslora).  Both sides are fp32 and differ only in summation order.  Measured max |diff| / max
    |logit|: 1.009e-6 (alpha_over_r, five targets) and 8.76e-7 (rslora, q and v); bound MERGED_REL_BOUND
    = 4 x 1.009e-6, far below 1e-3 of the logit scale.  (The difference grows with the adapter: with
    A and B three times larger it measured 8.0e-6 - rounding of the larger merged weights, no error.)"""
    transformers = pytest.importorskip("transformers")
    c = get_config("llama-tiny")
    r, alpha, targets, rs = (4, 8, ALL, False) if kind == "alpha_over_r" else (9, 6, ("q_proj", "v_proj"), True)
    sd = _write_peft_dir(tmp_path / "ad", c, r, alpha, targets, rs, seed=7)
    s = alpha / (r ** 0.5 if rs else r)
    base = CausalLM(c, device="cpu", dtype=torch.float32, seed=11)
    save_checkpoint(base, tmp_path / "base")
    hf = transformers.LlamaForCausalLM.from_pretrained(str(tmp_path / "base"), torch_dtype=torch.float32).eval()
    with torch.no_grad():
        for i in range(c.n_layers):
            for m in targets:
                parent = "self_attn" if m in ATTN else "mlp"
                p = f"base_model.model.model.layers.{i}.{parent}.{m}."
                w = getattr(getattr(hf.model.layers[i], parent), m).weight
                w.copy_((w.double() + s * (sd[p + "lora_B.weight"].double() @ sd[p + "lora_A.weight"].double())).float())
    ad = load_lora(tmp_path / "ad")
    assert abs(ad.scaling - s) < 1e-12
    base.enable_lora(2, 16)
    base.load_adapter(1, ad)
    ids = [1, 17, 33, 250, 5, 99, 140, 7, 61, 200, 3, 45, 300, 12, 90, 41, 8, 77]
    ours = _prefill_logits(base, ids, slot=1)
    with torch.no_grad():
        ref = hf(torch.tensor([ids])).logits[0].float()
    plain = _prefill_logits(base, ids)
    scale = ref.abs().max().item()
    rel = (ours - ref).abs().max().item() / scale
    print(f"{kind}: adapter path vs merged transformers model: max |diff| / max |logit| = {rel:.3e}; "
          f"base vs merged {(plain - ref).abs().max().item() / scale:.3e}")
    assert rel <= MERGED_REL_BOUND
    assert (plain - ref).abs().max().item() / scale > 1e3 * MERGED_REL_BOUND  # the adapter is no no-op
    # and merge_lora builds the same model
    merged = CausalLM(c, device="cpu", dtype=torch.float32, seed=11)
    merge_lora(merged, ad)
    assert (_prefill_logits(merged, ids) - ref).abs().max().item() / scale <= MERGED_REL_BOUND


# ------------------------------------------------------------------ 3. / 4. the engine

PROMPTS = ([7 + (5 * i) % 300 for i in range(23)], [11 + (7 * i) % 290 for i in range(20)],
           [3 + (11 * i) % 310 for i in range(27)])
STEPS = 8


@pytest.fixture(scope="module")
def adapter_dirs(tmp_path_factory):
    c = get_config("llama-tiny")
    root = tmp_path_factory.mktemp("adapters")
    a = _adapter(c, 4, ALL, 21, name="a")
    b = _adapter(c, 8, ("q_proj", "v_proj", "down_proj"), 22, rslora=True, name="b")
    return {"a": str(save_lora(a, root / "a")), "b": str(save_lora(b, root / "b"))}


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


def test_engine_mixed_batch_matches_merged_engines(adapter_dirs):
    eng = _engine(adapter_dirs)
    st = eng.stats()
    assert st["lora_enabled"] is False and st["lora_bytes"] == eng.model.lora.nbytes > 0
    assert st["lora_adapters"] == [
        {"name": "a", "rank": 4, "targets": sorted(ALL)},
        {"name": "b", "rank": 8, "targets": ["down_proj", "q_proj", "v_proj"]}]
    mixed = [s.output_ids for s in _run(eng, list(zip(PROMPTS, ("a", "b", None))))]
    assert eng.stats()["lora_enabled"] is True
    oracle = []
    for i, name in enumerate(("a", "b", None)):
        m = _engine()
        if name is not None:
            merge_lora(m.model, load_lora(adapter_dirs[name]))
        toks = _run(m, [(PROMPTS[i], None)])[0].output_ids
        # on the merged model alone: every compared step's top-2 margin is far above summation order
        for j in range(STEPS):
            lg = fp32_logits(m.model, torch.tensor(PROMPTS[i] + toks[:j]))[0]
            top = lg.topk(2).values
            assert int(lg.argmax()) == toks[j]
            assert (top[0] - top[1]).item() > 100 * MERGED_REL_BOUND * lg.abs().max().item(), (name, j)
        oracle.append(toks)
    assert mixed == oracle
    base_for_a = _run(_engine(), [(PROMPTS[0], None)])[0].output_ids
    assert base_for_a != oracle[0], "adapter a must change the tokens (a no-op implementation passes nothing)"


def test_no_adapters_configured_changes_nothing():
    eng = _engine()
    st = eng.stats()
    assert (st["lora_enabled"], st["lora_adapters"], st["lora_bytes"]) == (False, [], 0)
    assert eng.model.lora is None and eng.runner.d_lslot is None


def test_prefix_cache_is_per_adapter(adapter_dirs):
    eng = _engine(adapter_dirs)
    p = [9 + (3 * i) % 200 for i in range(40)]  # two full 16-token blocks

    def cached(e, ad):
        """Prompt tokens the admission took from the prefix cache (Sequence.num_cached, which the
        block manager clears again when the sequence finishes: read from its cumulative count)."""
        before = e.blocks.cached_tokens
        _run(e, [(p, ad)])
        return e.blocks.cached_tokens - before

    assert cached(eng, "a") == 0
    assert cached(eng, "a") == 32
    eng2 = _engine(adapter_dirs)
    assert [cached(eng2, ad) for ad in (None, "a", "b")] == [0, 0, 0]
    assert [cached(eng2, ad) for ad in (None, "a", "b")] == [32, 32, 32]


# ------------------------------------------------------------------ 5. refusals

def test_model_refusals(tmp_path):
    from k8s_llm_monitor_amd.parallel.state import ParallelState

    c = get_config("llama-tiny")
    ps = ParallelState(rank=0, world_size=2, tp_size=2, tp_rank=0, dp_rank=0, device=torch.device("cpu"))
    with pytest.raises(ValueError, match="tp_size"):
        CausalLM(c, device="cpu", dtype=torch.float32, pstate=ps).enable_lora(1)
    with pytest.raises(ValueError, match="gpt2"):
        CausalLM(get_config("gpt2-tiny"), device="cpu", dtype=torch.float32).enable_lora(1)
    m = CausalLM(c, device="cpu", dtype=torch.float32)
    m.enable_lora(1, 8)
    for t in ("gate_proj", "up_proj"):
        with pytest.raises(ValueError, match="SwiGLU"):
            m.load_adapter(0, _adapter(c, 4, (t,), 1))
    with pytest.raises(ValueError, match="lora_max_rank"):
        m.load_adapter(0, _adapter(c, 9, ATTN, 1))
    bad = _adapter(c, 4, ATTN, 1)
    A, B = bad.tensors[(0, "k_proj")]
    bad.tensors[(0, "k_proj")] = (A, torch.cat([B, B]))  # k_proj with q_proj's output rows
    with pytest.raises(ValueError, match="do not match the base model"):
        m.load_adapter(0, bad)
    moe = CausalLM(get_config("mixtral-tiny"), device="cpu", dtype=torch.float32)
    moe.enable_lora(1, 8)
    with pytest.raises(ValueError, match="MoE"):
        moe.load_adapter(0, _adapter(moe.cfg, 4, ("down_proj",), 1))
    moe.load_adapter(0, _adapter(moe.cfg, 4, ATTN, 1))  # the attention targets are fine


@pytest.mark.parametrize("extra,why", [({"use_dora": True}, "use_dora"), ({"bias": "all"}, "bias"),
                                       ({"modules_to_save": ["lm_head"]}, "modules_to_save")])
def test_adapter_config_refusals(tmp_path, extra, why):
    _write_peft_dir(tmp_path / "ad", get_config("llama-tiny"), 4, 8, ATTN, False, 1, cfg_extra=extra)
    with pytest.raises(ValueError, match=why):
        load_lora(tmp_path / "ad")


def test_unconsumed_adapter_tensors_are_an_error(tmp_path):
    _write_peft_dir(tmp_path / "ad", get_config("llama-tiny"), 4, 8, ATTN, False, 1,
                    extra_tensors={"base_model.model.lm_head.weight": torch.zeros(2, 2)})
    with pytest.raises(ValueError, match="not consumed"):
        load_lora(tmp_path / "ad")


def test_engine_refusals(adapter_dirs, tmp_path):
    with pytest.raises(ValueError, match="lora_max_rank"):
        _engine(adapter_dirs, lora_max_rank=4)
    eng = _engine(adapter_dirs)
    with pytest.raises(ValueError, match="unknown adapter 'nope'"):
        eng.add_request([1, 2, 3], SamplingParams(adapter="nope"))
    with pytest.raises(ValueError, match="unknown adapter"):
        _engine().add_request([1, 2, 3], SamplingParams(adapter="a"))


def test_http_adapter_fields(adapter_dirs):
    """/api/v1/query "adapter", /api/v1/analyze parameters.adapter (else llm.analysis_adapters) and the
    chat route's model-name convention; an unknown adapter is a 400 (tests/test_api.py style)."""
    from k8s_llm_monitor_amd.monitor.app import build_monitor
    from k8s_llm_monitor_amd.monitor.cluster.fake import FakeCluster
    from k8s_llm_monitor_amd.monitor.config import from_dict

    cfg = from_dict({"k8s": {"watch_namespaces": "default"}, "metrics": {"namespaces": ["default"]},
                     "llm": {"provider": "local-rocm", "model": "llama-tiny", "dtype": "float32", "max_batch": 4,
                             "max_model_len": 512, "kv_cache_gb": 0.01, "use_graphs": False, "max_tokens": 3,
                             "temperature": 0.0, "lora_adapters": adapter_dirs, "lora_max_rank": 16,
                             "analysis_adapters": {"root_cause": "b"}}})
    m = build_monitor(cfg, backend=FakeCluster.build(seed=2), start_manager=False, llm=True, device="cpu")
    try:
        m.manager.collect()
        app = m.app
        seen = []
        real = m.engine.add_request

        def spy(prompt, params=None, *a, **kw):
            seen.append(params.adapter if params is not None else None)
            return real(prompt, params, *a, **kw)

        m.engine.add_request = spy

        def post(path, body):
            r = app.handle("POST", path, json.dumps(body).encode())
            return r.code, r.body

        assert post("/api/v1/query", {"question": "why?", "adapter": "nope"})[0] == 400
        assert b"unknown adapter" in post("/api/v1/query", {"question": "why?", "adapter": "nope"})[1]
        assert post("/api/v1/query", {"question": "why?", "adapter": 3})[0] == 400
        assert post("/api/v1/analyze", {"type": "root_cause", "parameters": {"adapter": "nope"}})[0] == 400
        assert seen == []
        assert post("/api/v1/query", {"question": "why?", "adapter": "a", "max_tokens": 2})[0] == 200
        assert post("/api/v1/query", {"question": "why?", "max_tokens": 2})[0] == 200
        assert post("/api/v1/analyze", {"type": "root_cause", "parameters": {"max_tokens": 2}})[0] == 200
        assert post("/api/v1/analyze", {"type": "root_cause", "parameters": {"max_tokens": 2, "adapter": "a"}})[0] == 200
        assert post("/api/v1/analyze", {"type": "anomaly_detection", "parameters": {"max_tokens": 2}})[0] == 200
        chat = {"messages": [{"role": "user", "content": "hi"}], "max_tokens": 2}
        code, body = post("/v1/chat/completions", {**chat, "model": "a"})
        assert code == 200 and json.loads(body)["model"] == "a"
        code, body = post("/v1/chat/completions", {**chat, "model": "gpt-4"})
        assert code == 200 and json.loads(body)["model"] == "llama-tiny"
        assert seen == ["a", None, "b", "a", None, "a", None]
        d = json.loads(app.handle("GET", "/api/v1/metrics/engine").body)
        flat = json.dumps(d)
        assert '"lora_enabled": true' in flat and '"lora_bytes"' in flat and '"lora_adapters"' in flat
    finally:
        if m.engine_service is not None:
            m.engine_service.close()

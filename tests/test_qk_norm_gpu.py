"""QK-norm (Qwen3) on the GPU: the NORM form of rope_cache_kernel against the fp32 reference at
every compiled form (D 128 / 64, bf16 rows / split-K slabs, the fp8 cache's form), and a Qwen3
model served by the engine - a transformers checkpoint against the fp32 transformers model, and
chunked prefill beside decoding rows against the fp32 CPU model."""
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
F8 = torch.float8_e4m3fn
T, NB, BS = 50, 16, 16
EPS = 1e-4
# (Hq, Hkv, D): six workgroups per token | one partly filled workgroup (lanes past n_total) |
# 32 rope items + 8 V items in one wave, two heads in 16 lanes | D = 64 at a realistic head count
SHAPES = [(32, 8, 128), (2, 1, 128), (3, 1, 64), (16, 4, 64)]


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()


def _close(a, b, what, atol=2e-2, rtol=1e-2):  # the bounds of test_ops_gpu.py::test_rope_and_cache
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    bad = int((err > atol + rtol * b.abs()).sum())
    assert bad == 0, f"{what}: {bad} of {err.numel()} out of tolerance, max err {float(err.max()):.4g}"


def _inputs(hq, hkv, D, wdtype=torch.float32, seed=0):
    """CPU tensors: rows whose head h is scaled by 2^(h % 5) (a sum that crosses a head boundary
    is grossly wrong), one token's k head at 1e-3 (eps = 1e-4 matters), random positions, one slot
    -1, norm weights from [0.5, 2], different for q and k."""
    g = torch.Generator().manual_seed(100 + seed)
    ncol = (hq + 2 * hkv) * D
    x = torch.randn(T, ncol, generator=g)
    for h in range(hq + 2 * hkv):
        x[:, h * D:(h + 1) * D] *= 2.0 ** (h % 5)
    x[7, hq * D:(hq + 1) * D] = torch.randn(D, generator=g) * 1e-3
    pos = torch.randint(0, 4000, (T,), generator=g).to(torch.int32)
    slots = torch.randperm(NB * BS, generator=g)[:T].to(torch.int32)
    slots[3] = -1
    qw = (torch.rand(D, generator=g) * 1.5 + 0.5).to(wdtype)
    kw = (torch.rand(D, generator=g) * 1.5 + 0.5).to(wdtype)
    kc = torch.randn(NB, hkv, D // 8, BS, 8, generator=g).to(torch.bfloat16)
    vc = torch.randn(NB, hkv, D, BS, generator=g).to(torch.bfloat16)
    cs = ref.rope_cos_sin(4096, D, 1e6)
    return x, pos, slots, qw, kw, kc, vc, cs


def _slab_split(x, S, seed):
    """S fp32 slabs and the bf16 rows that hold their sum, added in the kernel's order."""
    g = torch.Generator().manual_seed(200 + seed)
    parts = [torch.randn(x.shape, generator=g) * x.abs().clamp(min=1e-3) for _ in range(S - 1)]
    last = x.clone()
    for p in parts:
        last -= p
    parts.append(last)
    part = torch.stack(parts)
    acc = part[0].clone()
    for s in range(1, S):
        acc += part[s]
    return part, acc.to(torch.bfloat16)


def _unwritten_equal(kc, vc, kc0, vc0, slots):
    """Every cache element outside the written slots is bit-equal to its earlier content."""
    keep = torch.ones(NB * BS, dtype=torch.bool)
    keep[slots[slots >= 0].long()] = False
    blk, off = torch.arange(NB * BS) // BS, torch.arange(NB * BS) % BS
    blk, off = blk[keep], off[keep]
    kc, vc = kc.cpu(), vc.cpu()
    assert torch.equal(kc[blk, :, :, off, :], kc0[blk, :, :, off, :]), "k cache outside the written slots"
    voff = ref.v_perm(off)
    assert torch.equal(vc[blk, :, :, voff], vc0[blk, :, :, voff]), "v cache outside the written slots"


@pytest.mark.parametrize("wdtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hq,hkv,D", SHAPES)
def test_qk_norm_matches_fp32_reference(hq, hkv, D, wdtype):
    x, pos, slots, qw, kw, kc0, vc0, cs = _inputs(hq, hkv, D, wdtype)
    want, kw_c, vw_c = x.to(torch.bfloat16), kc0.clone(), vc0.clone()
    ref.rope_and_cache(want, pos, cs, kw_c, vw_c, slots, hq, hkv, D, qk_norm=(qw, kw, EPS))
    got, kc, vc = x.to(torch.bfloat16).to(DEV), kc0.to(DEV), vc0.to(DEV)
    ops.rope_and_cache(got, pos.to(DEV), cs.to(DEV), kc, vc, slots.to(DEV), hq, hkv, D,
                       qk_norm=(qw.to(DEV), kw.to(DEV), EPS))
    torch.cuda.synchronize()
    plain = x.to(torch.bfloat16)
    ref.rope_and_cache(plain, pos, cs, None, None, None, hq, hkv, D)
    assert float((want.float() - plain.float()).abs().max()) > 1.0, "the norm changes the rows"
    _close(got, want, "qkv rows")
    _close(kc, kw_c, "k cache")
    assert torch.equal(got[:, (hq + hkv) * D:].cpu(), x.to(torch.bfloat16)[:, (hq + hkv) * D:]), "v columns"
    assert torch.equal(vc.cpu(), vw_c), "v cache"
    _unwritten_equal(kc, vc, kc0, vc0, slots)
    # without a cache: rows only, the same rows
    rows = x.to(torch.bfloat16).to(DEV)
    ops.rope_and_cache(rows, pos.to(DEV), cs.to(DEV), None, None, None, hq, hkv, D, qk_norm=(qw.to(DEV), kw.to(DEV), EPS))
    assert torch.equal(rows, got)
    # norm without rotation (the launch that a plain call would skip)
    got_n, kc_n, vc_n = x.to(torch.bfloat16).to(DEV), kc0.to(DEV), vc0.to(DEV)
    ops.rope_and_cache(got_n, pos.to(DEV), cs.to(DEV), kc_n, vc_n, slots.to(DEV), hq, hkv, D, apply_rope=False,
                       qk_norm=(qw.to(DEV), kw.to(DEV), EPS))
    want_n = x.to(torch.bfloat16)
    ref.rope_and_cache(want_n, pos, cs, None, None, None, hq, hkv, D, False, qk_norm=(qw, kw, EPS))
    _close(got_n, want_n, "rows, norm only")


@pytest.mark.parametrize("nslabs", [1, 3])
@pytest.mark.parametrize("hq,hkv,D", SHAPES)
def test_qk_norm_from_slabs_is_bit_identical_to_the_rows_form(hq, hkv, D, nslabs):
    """The kernel rounds the slab sum to bf16 first, so the slab form (which also writes the cache
    itself) == the form over bf16 rows holding that sum (whose cache write is the run-wise
    kernel's): rows and caches, bit for bit."""
    x, pos, slots, qw, kw, kc0, vc0, cs = _inputs(hq, hkv, D, seed=nslabs)
    part, rows = _slab_split(x, nslabs, nslabs)
    qk = (qw.to(DEV), kw.to(DEV), EPS)
    a, kca, vca = torch.zeros_like(rows).to(DEV), kc0.to(DEV), vc0.to(DEV)
    ops.rope_and_cache(a, pos.to(DEV), cs.to(DEV), kca, vca, slots.to(DEV), hq, hkv, D,
                       partial=part.to(DEV).reshape(-1), nslabs=nslabs, qk_norm=qk)
    b, kcb, vcb = rows.to(DEV), kc0.to(DEV), vc0.to(DEV)
    ops.rope_and_cache(b, pos.to(DEV), cs.to(DEV), kcb, vcb, slots.to(DEV), hq, hkv, D, qk_norm=qk)
    torch.cuda.synchronize()
    nqk = (hq + hkv) * D
    assert torch.equal(a[:, :nqk], b[:, :nqk]), "q / k rows"
    assert torch.equal(kca, kcb), "k cache"
    assert torch.equal(vca, vcb), "v cache"
    _unwritten_equal(kca, vca, kc0, vc0, slots)
    want = rows.clone()
    ref.rope_and_cache(want, pos, cs, None, None, None, hq, hkv, D, qk_norm=(qw, kw, EPS))
    _close(a[:, :nqk], want[:, :nqk], "q / k rows against the reference")


@pytest.mark.parametrize("nslabs", [0, 3])
@pytest.mark.parametrize("hq,hkv", [(32, 8), (2, 1)])
def test_qk_norm_fp8_cache_holds_quantize_kv_of_the_rows(hq, hkv, nslabs):
    """fp8 cache (D = 128): codes and scales == ops.quantize_kv of the rows the same call left in
    qkv, bit for bit (compared as tests/test_kv_fp8_gpu.py compares the plain form); every other
    byte and scale keeps its sentinel."""
    D = 128
    x, pos, slots, qw, kw, _, _, cs = _inputs(hq, hkv, D, seed=7 + nslabs)

    def sentinel(device):
        k, v, sc = (t[0] for t in ops.kv_cache_alloc(1, NB, hkv, D, F8, device))
        k.view(torch.uint8).fill_(0x5A)
        v.view(torch.uint8).fill_(0x5A)
        sc.fill_(7.0)
        return k, v, sc

    got, want = sentinel(DEV), sentinel("cpu")
    qk = (qw.to(DEV), kw.to(DEV), EPS)
    if nslabs:
        part, rows = _slab_split(x, nslabs, 9)
        qkv = torch.zeros_like(rows).to(DEV)
        ops.rope_and_cache(qkv, pos.to(DEV), cs.to(DEV), got[0], got[1], slots.to(DEV), hq, hkv, D,
                           partial=part.to(DEV).reshape(-1), nslabs=nslabs, kv_scale=got[2], qk_norm=qk)
    else:
        rows = x.to(torch.bfloat16)
        qkv = rows.to(DEV)
        ops.rope_and_cache(qkv, pos.to(DEV), cs.to(DEV), got[0], got[1], slots.to(DEV), hq, hkv, D, kv_scale=got[2],
                           qk_norm=qk)
    torch.cuda.synchronize()
    expect = rows.clone()
    ref.rope_and_cache(expect, pos, cs, None, None, None, hq, hkv, D, qk_norm=(qw, kw, EPS))
    _close(qkv, expect, "rows")
    k = qkv[:, hq * D:(hq + hkv) * D].reshape(T, hkv, D).cpu()
    v = qkv[:, (hq + hkv) * D:].reshape(T, hkv, D).cpu()
    assert torch.equal(v, rows[:, (hq + hkv) * D:].reshape(T, hkv, D)), "v rows"
    ref.write_kv_cache(k, v, want[0], want[1], slots, want[2])
    for g, w, n in zip(got, want, ("k codes", "v codes", "scales")):
        g = g.cpu()
        assert torch.equal(g.float(), w.float()), f"{n} differ at {int((g.float() != w.float()).sum())} places"
    assert int((got[2] == 7.0).sum()) == got[2].numel() - (T - 1) * hkv * 2, "only the written tokens' scales moved"


@pytest.mark.parametrize("hq,hkv,D", [(32, 8, 128), (3, 1, 64)])
def test_default_is_unchanged(hq, hkv, D):
    """qk_norm=None == the argument left out: rows and caches, bit for bit, rows and slabs."""
    x, pos, slots, _, _, kc0, vc0, cs = _inputs(hq, hkv, D, seed=3)
    part, rows = _slab_split(x, 2, 3)
    outs = []
    for kw in ({}, {"qk_norm": None}):
        for sl in (False, True):
            q, kc, vc = rows.to(DEV), kc0.to(DEV), vc0.to(DEV)
            extra = dict(partial=part.to(DEV).reshape(-1), nslabs=2) if sl else {}
            ops.rope_and_cache(q, pos.to(DEV), cs.to(DEV), kc, vc, slots.to(DEV), hq, hkv, D, **extra, **kw)
            outs.append((q, kc, vc))
    for a, b in ((outs[0], outs[2]), (outs[1], outs[3])):
        assert all(torch.equal(s, t) for s, t in zip(a, b))


def test_binding_refuses_bad_norm_weights():
    hq, hkv, D = 2, 1, 128
    x, pos, slots, qw, kw, _, _, cs = _inputs(hq, hkv, D)
    q = x.to(torch.bfloat16).to(DEV)
    nat = ops.native()
    e = torch.empty(0, dtype=torch.int32, device=DEV)
    args = (q, pos.to(DEV), cs.to(DEV), e, e, e, hq, hkv, D, True, None, 0, None)
    for bad in ((qw.to(DEV)[:64], kw.to(DEV)), (qw, kw), (qw.to(DEV), kw.to(DEV).bfloat16()), (qw.to(DEV).half(), kw.to(DEV).half()),
                (qw.to(DEV), None)):
        with pytest.raises(RuntimeError):
            nat.rope_and_cache(*args, bad[0], bad[1], EPS)
    with pytest.raises(ValueError):
        ops.rope_and_cache(q, pos.to(DEV), cs.to(DEV), None, None, None, hq, hkv, D, qk_norm=(qw, kw.to(DEV), EPS))
    assert torch.equal(q.cpu(), x.to(torch.bfloat16)), "a refused call writes nothing"


# ------------------------------------------------------------------ the engine
PROMPTS = [[1, 17, 33, 250, 5, 99, 140, 7, 61, 200, 3, 45] * 3, [1, 900, 12, 12, 4, 700, 31]]
N_NEW = 12


def _agreement(outs, wants):
    """tests/test_checkpoint.py's count: tokens up to and including a prompt's first difference."""
    agree = total = 0
    for got, want in zip(outs, wants):
        for a, b in zip(got, want):
            total += 1
            agree += int(a == b)
            if a != b:
                break
    return agree, total


@pytest.fixture(scope="module")
def hf_run(tmp_path_factory):
    """A transformers Qwen3 checkpoint (2 layers, hidden 512, 8 / 2 heads, head_dim 128, vocab 1024,
    every parameter random, the 2-d weights times 3 for decisive logits), the fp32 model's greedy
    tokens, and the engines' tokens per serving mode (each engine is built once)."""
    transformers = pytest.importorskip("transformers")
    from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams

    path = tmp_path_factory.mktemp("qwen3")
    torch.manual_seed(0)
    cfg = transformers.Qwen3Config(vocab_size=1024, hidden_size=512, intermediate_size=1024, num_hidden_layers=2,
                                   num_attention_heads=8, num_key_value_heads=2, head_dim=128,
                                   max_position_embeddings=1024, rope_theta=1e6, rms_norm_eps=1e-6,
                                   tie_word_embeddings=False, bos_token_id=1, eos_token_id=2)
    hf = transformers.Qwen3ForCausalLM(cfg)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for n, p in hf.named_parameters():
            if p.dim() == 1:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.mul_(3.0)
    hf = hf.float().eval()
    hf.save_pretrained(path, safe_serialization=True)
    wants = []
    for p in PROMPTS:
        with torch.no_grad():
            wants.append(hf.generate(torch.tensor([p]), max_new_tokens=N_NEW, do_sample=False,
                                     attention_mask=torch.ones(1, len(p), dtype=torch.long))[0, len(p):].tolist())
    served = {}

    def serve(kind):
        if kind not in served:
            kw = {"graphs": {}, "eager": {"use_graphs": False}, "fp8": {"kv_cache_dtype": "fp8"}}[kind]
            eng = LLMEngine(EngineConfig(weights=str(path), max_num_seqs=4, max_model_len=512, num_blocks=64, seed=0,
                                         **kw), device="cuda:0")
            assert eng.model_cfg.qk_norm and not eng.model._attn_rope
            assert not eng.model._fused_norm_ok(torch.empty(4096, 512, device="cuda:0", dtype=torch.bfloat16))
            eng.warmup()
            assert bool(eng.runner.graphs) == (kind != "eager")
            if kind == "fp8":
                assert eng.runner.kv_cache_dtype == "fp8"
            seqs = eng.generate(PROMPTS, SamplingParams(max_tokens=N_NEW, temperature=0.0, ignore_eos=True))
            torch.cuda.synchronize()
            served[kind] = [list(s.output_ids) for s in seqs]
        return served[kind]

    return wants, serve


@pytest.mark.parametrize("kind", ["graphs", "eager", "fp8"])
def test_engine_on_hf_qwen3_checkpoint_matches_transformers(hf_run, kind):
    wants, serve = hf_run
    outs = serve(kind)
    assert all(len(o) == N_NEW for o in outs)
    agree, total = _agreement(outs, wants)
    print(f"{kind}: {agree} of {total} compared tokens agree with the fp32 transformers model")
    assert agree >= 0.8 * total, (agree, total)


def test_engine_graphs_on_and_off_produce_the_same_tokens(hf_run):
    _, serve = hf_run
    assert serve("graphs") == serve("eager")


def test_mixed_steps_and_chunked_prefill_match_the_fp32_cpu_model():
    """qwen3-tiny-d128 with a 48-token prefill budget: a long prompt arrives while two short ones
    decode, so it prefills in chunks (later chunks attend the earlier ones from the cache) in steps
    that also carry decode rows.  The fp32 CPU engine on the same weights, driven the same way, is
    the reference; agreement by the checkpoint test's rule."""
    from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams

    def drive(eng):
        sp = SamplingParams(max_tokens=N_NEW, temperature=0.0, ignore_eos=True)
        seqs = [eng.add_request(p, sp) for p in ("node NotReady", "pod default/api-gateway crashloop")]
        for _ in range(2):
            eng.step()
        seqs.append(eng.add_request("集群状态概览: node-001 CPU=93.1% [资源压力] why is coredns failing " * 6, sp))
        while eng.has_work():
            eng.step()
        return [list(s.output_ids) for s in seqs]

    kw = dict(model="qwen3-tiny-d128", max_num_seqs=4, max_model_len=512, num_blocks=128, seed=4,
              max_prefill_tokens=48, mixed_prefill_tokens=48, prefix_caching=False)
    gpu = LLMEngine(EngineConfig(**kw), device="cuda:0")
    gpu.warmup()
    outs = drive(gpu)
    torch.cuda.synchronize()
    assert gpu.counters["mixed_steps"] > 0 and gpu.runner.n_steps["prefill_context_tokens"] > 0
    assert not gpu.tokenizer.add_bos
    cpu = LLMEngine(EngineConfig(**kw, use_graphs=False, dtype="float32"), device="cpu")
    cpu.model.copy_weights_from(gpu.model)
    wants = drive(cpu)
    assert cpu.counters["mixed_steps"] > 0
    agree, total = _agreement(outs, wants)
    print(f"mixed / chunked: {agree} of {total} compared tokens agree with the fp32 CPU model")
    assert agree >= 0.8 * total, (agree, total)

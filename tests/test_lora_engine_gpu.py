"""Per-request LoRA adapters through the model and the engine on the GPU (llama-tiny-d128 and
qwen3-tiny-d128, two adapters).  The oracle is the merged model: models/reference.py fp32_logits of
an fp32 CPU copy of the GPU model's (dequantised) weights with W + s B A folded in.

Criterion (tests 1-3): the base rows' max error / logit scale against fp32_logits of the base model -
the smoke test's quantity - is measured in the same test, and the adapter rows may exceed it by at
most a factor of 2: each adapted projection output takes one extra bf16 rounding (or one more fp32
slab in the sum), of the same size as the roundings already there.  The adapters are scaled so that
merged and base logits differ by at least 20 times that error, asserted on the references alone."""
import functools

import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.engine.runner import ModelRunner, RunnerConfig
from k8s_llm_monitor_amd.models.checkpoint import LoraAdapter, merge_lora, save_lora
from k8s_llm_monitor_amd.models.config import get_config
from k8s_llm_monitor_amd.models.llama import AttnMeta, CausalLM
from k8s_llm_monitor_amd.models.reference import fp32_logits

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS = 8
BPS = 4  # KV blocks per sequence (64 tokens)
ALL = ("q_proj", "k_proj", "v_proj", "o_proj", "down_proj")
KINDS = ("a", "b", None)  # rows cycle through adapter a, adapter b and the base model


@pytest.fixture(autouse=True, scope="module")
def _native_loaded():
    ops.native()
    yield
    _adapters.cache_clear()


@functools.lru_cache(maxsize=None)
def _adapters(model_name, gain=1.0):
    """Adapters a and b; ``gain`` scales both (the fp8 KV cache's larger base error needs larger adapters
    for the 20 x separation)."""
    c = get_config(model_name)
    D, d = c.head_dim, c.d_model
    shapes = {"q_proj": (c.n_heads * D, d), "k_proj": (c.n_kv_heads * D, d), "v_proj": (c.n_kv_heads * D, d),
              "o_proj": (d, c.n_heads * D), "down_proj": (d, c.ffn_dim)}
    out = {}
    for name, r, targets, rs, seed in (("a", 16, ALL, False, 31), ("b", 8, ("q_proj", "v_proj", "down_proj"), True, 32)):
        g = torch.Generator().manual_seed(seed)
        t = {}
        for layer in range(c.n_layers):
            for m in targets:
                o, i = shapes[m]
                t[(layer, m)] = ((torch.randn(r, i, generator=g) * 0.05).to(torch.bfloat16),
                                 (torch.randn(o, r, generator=g) * 0.05).to(torch.bfloat16))
        # scalings 8 / 16 and 2 / sqrt(8): merged and base logits differ by about a quarter of the logit scale
        out[name] = LoraAdapter(r=r, lora_alpha=gain * {"a": 8.0, "b": 2.0}[name], target_modules=tuple(sorted(targets)),
                                tensors=t, use_rslora=rs, name=name)
    return out


class Harness:
    """A GPU model with both adapters resident, a paged KV cache, and the fp32 CPU references: the
    base model and one merged model per adapter, over the GPU model's own (dequantised) weights."""

    def __init__(self, model_name, rows, dec_weights="bf16", kv="bf16", gain=1.0):
        c = get_config(model_name)
        self.c, self.B = c, rows
        self.model = CausalLM(c, device=DEV, seed=3, dec_weights=dec_weights)
        self.model.enable_lora(2, 16)
        ads = _adapters(model_name, gain)
        for slot, name in enumerate(("a", "b")):
            self.model.load_adapter(slot, ads[name])
        self.runner = ModelRunner(self.model, RunnerConfig(max_num_seqs=rows, max_model_len=16 * BPS,
                                                           num_blocks=rows * BPS + 1, use_graphs=False,
                                                           kv_cache_dtype=kv))
        self.refs = {}
        for name in KINDS:
            ref = CausalLM(c, device="cpu", dtype=torch.float32, seed=3)
            ref.copy_weights_from(self.model)
            if name is not None:
                merge_lora(ref, ads[name])
            self.refs[name] = ref
        self.kinds = [KINDS[i % 3] for i in range(rows)]
        self.slots = [{"a": 0, "b": 1, None: -1}[k] for k in self.kinds]
        self.seqs = [[1] + [5 + (7 * i + 13 * j) % 1000 for j in range(5 + i % 8)] for i in range(rows)]
        self.bt = torch.tensor([[1 + BPS * i + j for j in range(BPS)] for i in range(rows)], dtype=torch.int32,
                               device=DEV)

    def _slot_of(self, i, p):
        return int(self.bt[i, p // 16]) * 16 + p % 16

    def prefill(self):
        """One prefill step over every prompt: logits of each prompt's last row [B, V]."""
        ids, pos, sm, ls, cu = [], [], [], [], [0]
        for i, s in enumerate(self.seqs):
            ids += s
            pos += list(range(len(s)))
            sm += [self._slot_of(i, p) for p in range(len(s))]
            ls += [self.slots[i]] * len(s)
            cu.append(cu[-1] + len(s))
        t = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)  # noqa: E731
        meta = AttnMeta(is_prefill=True, positions=t(pos), slot_mapping=t(sm), cu_seqlens=t(cu),
                        logits_idx=(t(cu)[1:] - 1).long(), lora_slot=t(ls))
        with torch.no_grad():
            return self.model.forward(t(ids), meta, self.runner.kv).float().cpu()

    def decode(self, first_tokens):
        """STEPS greedy decode steps, each run eagerly and as a captured graph over the same static
        inputs: asserts the two logits bit-identical, returns the steps' logits [STEPS, B, V]."""
        B = self.B
        z = lambda: torch.zeros(B, dtype=torch.int32, device=DEV)  # noqa: E731
        d_ids, d_pos, d_sm, d_len = z(), z(), z(), z()
        d_ls = torch.tensor(self.slots, dtype=torch.int32, device=DEV)
        meta = AttnMeta(is_prefill=False, positions=d_pos, slot_mapping=d_sm, block_tables=self.bt, seq_lens=d_len,
                        decode_ws=self.runner.decode_ws, lora_slot=d_ls)

        def fill(toks):
            n = [len(s) for s in self.seqs]
            d_ids.copy_(torch.tensor(toks, dtype=torch.int32))
            d_pos.copy_(torch.tensor([k - 1 for k in n], dtype=torch.int32))
            d_sm.copy_(torch.tensor([self._slot_of(i, k - 1) for i, k in enumerate(n)], dtype=torch.int32))
            d_len.copy_(torch.tensor(n, dtype=torch.int32))

        def body():
            with torch.no_grad():
                return self.model.forward(d_ids, meta, self.runner.kv)

        toks = list(first_tokens)
        for s, tk in zip(self.seqs, toks):
            s.append(tk)
        fill(toks)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            g_logits = body()
        out = []
        for _ in range(STEPS):
            eager = body().clone()
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(eager, g_logits), "a captured step's logits differ from the eager step's"
            out.append(eager.float().cpu())
            toks = eager.float().argmax(-1).tolist()
            for s, tk in zip(self.seqs, toks):
                s.append(tk)
            fill(toks)
        return torch.stack(out)

    def ref_logits(self, i, name, rows):
        return fp32_logits(self.refs[name], torch.tensor(self.seqs[i]), rows, device="cpu")


def _judge(h, got, rows_of, what):
    """``got[i]`` [n, V]: GPU logits of sequence i at its positions ``rows_of(i)``.  Base rows give the
    yardstick error; adapter rows stay within twice it, and differ from the base model by >= 20 x."""
    err = {k: 0.0 for k in KINDS}
    sep = 1e30
    for i, k in enumerate(h.kinds):
        ref = h.ref_logits(i, k, rows_of(i))
        scale = ref.abs().max().item()
        err[k] = max(err[k], (got[i] - ref).abs().max().item() / scale)
        if k is not None:
            base = h.ref_logits(i, None, rows_of(i))
            sep = min(sep, (ref - base).abs().amax(-1).min().item() / scale)
    print(f"{what}: max err / logit scale: base {err[None]:.5f}, adapter a {err['a']:.5f}, adapter b {err['b']:.5f}; "
          f"least merged-vs-base difference / scale {sep:.3f}")
    assert err[None] < 0.03, "the base rows miss the smoke test's own bound"
    assert sep >= 20 * err[None], "the adapters are too small for this comparison"
    assert err["a"] <= 2 * err[None] and err["b"] <= 2 * err[None]


@pytest.mark.parametrize("model_name", ["llama-tiny-d128", "qwen3-tiny-d128"])
def test_prefill_logits_match_merged_model(model_name):
    h = Harness(model_name, 9)
    got = h.prefill()
    _judge(h, [got[i:i + 1] for i in range(h.B)], lambda i: [len(h.seqs[i]) - 1], f"prefill {model_name}")


def _decode_case(model_name, rows, **kw):
    h = Harness(model_name, rows, **kw)
    T0 = [len(s) for s in h.seqs]
    first = h.prefill().argmax(-1).tolist()
    lg = h.decode(first)  # [STEPS, B, V]; step j of sequence i is position T0[i] + j
    _judge(h, [lg[:, i] for i in range(rows)], lambda i: list(range(T0[i], T0[i] + STEPS)),
           f"decode {model_name} rows={rows} {kw}")


@pytest.mark.parametrize("rows", [3, 40])
@pytest.mark.parametrize("model_name", ["llama-tiny-d128", "qwen3-tiny-d128"])
def test_decode_with_graphs_matches_merged_model(model_name, rows):
    _decode_case(model_name, rows)


@pytest.mark.parametrize("kw", [{"dec_weights": "fp8"}, {"kv": "fp8", "gain": 2.0}], ids=["decode_weights_fp8", "kv_cache_fp8"])
def test_decode_weight_and_cache_formats(kw):
    _decode_case("llama-tiny-d128", 3, **kw)


def test_base_traffic_is_unchanged(tmp_path):
    """Requests without an adapter give the same tokens before and after the first adapter request, and
    the tokens of an engine with no adapters configured; lora_enabled flips on that request only."""
    ads = _adapters("llama-tiny-d128")
    dirs = {n: str(save_lora(ads[n], tmp_path / n)) for n in ("a", "b")}
    prompts = [[1] + [9 + (11 * i + 3 * j) % 900 for j in range(12 + i)] for i in range(3)]

    def engine(adapters):
        e = LLMEngine(EngineConfig(model="llama-tiny-d128", max_num_seqs=8, max_model_len=256, num_blocks=128, seed=0,
                                   prefix_caching=False, lora_adapters=adapters), device="cuda:0")
        e.warmup()
        return e

    def run(e, adapter=None):
        seqs = [e.add_request(list(p), SamplingParams(max_tokens=STEPS, temperature=0.0, ignore_eos=True,
                                                      adapter=adapter)) for p in prompts]
        while e.has_work():
            e.step()
        return [s.output_ids for s in seqs]

    e = engine(dirs)
    before = run(e)
    assert e.stats()["lora_enabled"] is False and e.runner.graphs_lora == {}
    with_a = run(e, "a")
    assert e.stats()["lora_enabled"] is True and sorted(e.runner.graphs_lora) == sorted(e.runner.graphs)
    after = run(e)
    plain = engine({})
    assert plain.stats()["lora_bytes"] == 0 and plain.model.lora is None
    assert before == after == run(plain)
    assert with_a != before

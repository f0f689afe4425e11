"""Token log-probabilities on the GPU: logprobs.hip against the fp64 definition (ids exact, ties
included), inside a captured step, and through the engine with graphs and pipelined decode."""
import functools

import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, LLMEngine, SamplingParams
from test_logprobs_cpu import LP_TOL, SHAPES, ForwardSpy, check_sequence, make_logits

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x5A5A5A5A
WANT_CYCLE = (-1, 0, 1, 5, 20)


def parts(B, V):
    """k8sllm_sample_parts and the 8-aligned part length of sample_partial_row."""
    p = max(1, min((512 + B - 1) // B, max(V // 8192, 1)))
    return p, ((V + p - 1) // p + 7) // 8 * 8


def plant_ties(x):
    """Row 1: the top value occurs 30 times, spread over the first and the last part.  Row 2: 19
    distinct values on top, then the 20th and 21st largest are equal and lie in different parts
    (the later part holds the lower-ranked one only by its index)."""
    B, V = x.shape
    P, chunk = parts(B, V)
    assert P >= 2 and B >= 3
    last = (P - 1) * chunk
    idx = [7 + 11 * j for j in range(15)] + [last + 5 + 13 * j for j in range(15)]
    assert max(idx) < V
    x[1, idx] = 9.0
    top = [chunk // 2 + 17 * j for j in range(19)]
    x[2, top] = torch.tensor([20.0 - 0.5 * j for j in range(19)]).to(x.dtype)
    x[2, [chunk - 3, last + 1]] = 9.5
    return x


class Case:
    """bf16 logits [B, V] on the device in the three layouts the kernel reads, the tokens the
    sampler draws from them and the fp64 reference, computed once."""

    def __init__(self, B, V, ties=False):
        ops.native()
        x = make_logits(B, V)
        if ties:
            x = plant_ties(x)
        self.B, self.V = B, V
        stride = (V + 7) // 8 * 8 + 8
        buf = torch.zeros(B + 1, stride, dtype=torch.bfloat16)
        buf[:B, :V] = x
        shifted = torch.zeros(B + 1, stride, dtype=torch.bfloat16)
        shifted[1:, 3:3 + V] = x
        self.layouts = {"bf16 view": buf.to(DEV)[:B, :V], "fp32": x.float().to(DEV).contiguous(),
                        "bf16 unaligned": shifted.to(DEV)[1:, 3:3 + V]}
        assert self.layouts["bf16 view"].stride(0) != V and self.layouts["bf16 unaligned"].data_ptr() % 16 != 0
        temps = torch.tensor([0.0 if b % 2 == 0 else 0.9 for b in range(B)], device=DEV)
        rng = torch.tensor([11, 0], dtype=torch.int64, device=DEV)
        self.tok = ops.sample(self.layouts["bf16 view"], temps, None, None, rng)
        x64 = x.double()
        self.lps = torch.log_softmax(x64, -1)
        self.order = torch.sort(x64, descending=True, stable=True).indices[:, :ops.LP_MAX_TOP]

    def check(self, rec, want, tok):
        """The packed records of one launch against fp64; returns the largest finite error."""
        rec, tok, err = rec.cpu(), tok.cpu().tolist(), 0.0
        for b, n in enumerate(want):
            if n < 0:
                assert bool((rec[b] == SENTINEL).all())
                continue
            lp, top = ops.unpack_logprobs(rec[b])
            k = min(n, self.V)
            assert [i for i, _ in top] == self.order[b, :k].tolist(), (b, n)
            assert rec[b, 21 + k:].tolist() == [-1] * (20 - k)
            assert bool((rec[b, 1 + k:21].view(torch.float32) == float("-inf")).all())
            pairs = [(tok[b], lp)] + top
            ref = self.lps[b, [i for i, _ in pairs]].tolist()
            for (i, v), w in zip(pairs, ref):
                if w == float("-inf"):
                    assert v == w
                else:
                    assert abs(v - w) <= LP_TOL, (b, i, v, w)
                    err = max(err, abs(v - w))
        return err


@functools.lru_cache(maxsize=None)
def case(B, V, ties=False):
    return Case(B, V, ties)


def launch(c, logits, want):
    out = torch.full((c.B, ops.LP_WIDTH), SENTINEL, dtype=torch.int32, device=DEV)
    w = torch.tensor(want, dtype=torch.int32, device=DEV)
    return ops.token_logprobs(logits, c.tok, w, out=out)


# ---------------------------------------------------------------- 1. the kernel against the reference

@pytest.mark.parametrize("layout", ["bf16 view", "fp32", "bf16 unaligned"])
@pytest.mark.parametrize("B,V", SHAPES)
def test_kernel_matches_fp64(B, V, layout):
    c = case(B, V)
    logits = c.layouts[layout]
    err = 0.0
    for rot in range(len(WANT_CYCLE)):  # every row takes every want once
        want = [WANT_CYCLE[(b + rot) % len(WANT_CYCLE)] for b in range(B)]
        rec = launch(c, logits, want)
        err = max(err, c.check(rec, want, c.tok))
        if rot == 2:
            assert torch.equal(launch(c, logits, want), rec)  # bit-identical on every launch
    print(f"logprobs ({B}, {V}) {layout}: max |lp - fp64| = {err:.3e}")


@pytest.mark.parametrize("layout", ["bf16 view", "fp32", "bf16 unaligned"])
@pytest.mark.parametrize("B,V", [(3, 50257), (128, 32000)])
def test_kernel_planted_ties(B, V, layout):
    c = case(B, V, True)
    P, chunk = parts(B, V)
    # what the plan plants: row 1's 20 best are the 15 copies in part 0 and the first 5 of the last
    # part; row 2's 20th is the tie's lower index, in an earlier part than the 21st
    assert c.order[1].tolist() == [7 + 11 * j for j in range(15)] + [(P - 1) * chunk + 5 + 13 * j for j in range(5)]
    assert c.order[2, 19].item() == chunk - 3
    want = [20] * B
    rec = launch(c, c.layouts[layout], want)
    c.check(rec, want, c.tok)
    assert torch.equal(launch(c, c.layouts[layout], want), rec)


def test_kernel_more_parts_than_one_merge_pass():
    """A vocabulary large enough for 64 parts: the final kernel merges 63 lists per pass, so the
    last part meets the merged list of the others.  The top value sits in parts 0, 62 and 63."""
    B, V = 1, 64 * 8192 + 1001
    P, chunk = parts(B, V)
    assert P == 64
    c = Case.__new__(Case)
    x = make_logits(B, V)
    idx = [40 + 9 * j for j in range(10)] + [62 * chunk + 3 + 7 * j for j in range(5)] + \
          [63 * chunk + 11 * j for j in range(10)]
    x[0, idx] = 9.0
    c.B, c.V = B, V
    logits = x.to(DEV)
    c.tok = ops.sample(logits)
    c.lps = torch.log_softmax(x.double(), -1)
    c.order = torch.sort(x.double(), descending=True, stable=True).indices[:, :ops.LP_MAX_TOP]
    assert c.order[0].tolist() == idx[:20]
    for want in ([20], [5], [0]):
        rec = launch(c, logits, want)
        c.check(rec, want, c.tok)
        assert torch.equal(launch(c, logits, want), rec)


def test_binding_refuses_wrong_arguments():
    c = case(2, 1000)
    logits = c.layouts["bf16 view"]
    want = torch.zeros(2, dtype=torch.int32, device=DEV)
    out = torch.zeros(2, ops.LP_WIDTH, dtype=torch.int32, device=DEV)
    nat = ops.native()
    with pytest.raises(RuntimeError):
        nat.token_logprobs(out[:, :40], logits, c.tok, want)
    with pytest.raises(RuntimeError):
        nat.token_logprobs(out[:1], logits, c.tok, want)
    with pytest.raises(RuntimeError):
        nat.token_logprobs(out, logits, c.tok[:1], want)
    with pytest.raises(RuntimeError):
        nat.token_logprobs(out, logits, c.tok, want.long())
    with pytest.raises(RuntimeError):
        nat.token_logprobs(out, logits.half(), c.tok, want)


# ---------------------------------------------------------------- 2. a captured step

def test_captured_sample_and_logprobs_step():
    B, V = 4, 50257
    cases = [make_logits(B, V, seed=s) for s in (1, 2, 3)]
    wants = [[5, 0, -1, 20], [20, 20, 1, 0], [-1, 3, 5, 20]]
    stride = (V + 7) // 8 * 8 + 8
    buf = torch.zeros(B, stride, dtype=torch.bfloat16, device=DEV)
    logits = buf[:, :V]
    logits.copy_(cases[0])
    temps = torch.tensor([0.0, 0.7, 1.0, 0.0], device=DEV)
    rng = torch.tensor([5, 0], dtype=torch.int64, device=DEV)
    tok = torch.zeros(B, dtype=torch.int32, device=DEV)
    want = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    rec = torch.full((B, ops.LP_WIDTH), SENTINEL, dtype=torch.int32, device=DEV)

    def step():
        ops.sample(logits, temps, None, None, rng, out=tok, advance=True)
        ops.token_logprobs(logits, tok, want, out=rec)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert bool((rec == SENTINEL).all())  # want = -1 everywhere: nothing computed
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    for x, w in zip(cases, wants):
        logits.copy_(x)
        want.copy_(torch.tensor(w, dtype=torch.int32))
        rec.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        c = types_case(x)
        assert bool(((tok >= 0) & (tok < V)).all())
        c.check(rec, w, tok)


def types_case(x):
    """A reference-only Case over given logits (no device layouts)."""
    c = Case.__new__(Case)
    c.B, c.V = x.shape
    x64 = x.double()
    c.lps = torch.log_softmax(x64, -1)
    c.order = torch.sort(x64, descending=True, stable=True).indices[:, :ops.LP_MAX_TOP]
    return c


# ---------------------------------------------------------------- 3. the engine, graphs, pipelined decode

def test_engine_graphs_and_pipelined_decode():
    cfg = dict(model="llama-tiny-d128", max_num_seqs=8, max_model_len=1024, num_blocks=512, seed=3)
    prompts = ["kube-system coredns CrashLoopBackOff", "MEM=95.9% [资源压力]" * 20]
    lp = SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True, logprobs=True, top_logprobs=5)
    plain = SamplingParams(max_tokens=12, temperature=0.0, ignore_eos=True)

    a = LLMEngine(EngineConfig(**cfg, use_graphs=False), device="cuda")
    spy = ForwardSpy(a)
    sa = a.generate(prompts, lp)
    for s in sa:
        assert len(s.output_ids) == 12
        check_sequence(s, spy, 5)

    b = LLMEngine(EngineConfig(**cfg), device="cuda")
    b.warmup()
    assert b.runner.graphs and not b.runner.lp_on
    buckets, captures, capture = sorted(b.runner.graphs), [], b.runner.capture_graphs
    b.runner.capture_graphs = lambda bk=None: captures.append(bk) or capture(bk)
    sb = b.generate(prompts, lp)  # the first request arrives after warmup(): the graphs are captured again
    assert b.runner.lp_on and captures == [buckets] and sorted(b.runner.graphs) == buckets
    for x, y in zip(sa, sb):
        assert y.output_ids == x.output_ids
        assert len(y.output_logprobs) == len(y.output_ids)
        for ex, ey in zip(x.output_logprobs, y.output_logprobs):
            assert abs(ex[0] - ey[0]) <= LP_TOL
            assert [i for i, _ in ey[1]] == [i for i, _ in ex[1]]
            assert all(abs(vx - vy) <= LP_TOL for (_, vx), (_, vy) in zip(ex[1], ey[1]))

    never = LLMEngine(EngineConfig(**cfg), device="cuda")
    never.warmup()
    want = [s.output_ids for s in never.generate(prompts, plain)]
    assert not never.runner.lp_on and never.stats()["logprobs_enabled"] is False
    second = b.generate(prompts, plain)  # enabled, nobody asks
    assert [s.output_ids for s in second] == want and all(s.output_logprobs is None for s in second)
    s0, s1 = b.add_request(prompts[0], plain), b.add_request(prompts[1], lp)  # one row asks, its neighbour not
    while b.has_work():
        b.step()
    assert [s0.output_ids, s1.output_ids] == want and s0.output_logprobs is None
    assert captures == [buckets]  # once
    assert [[i for i, _ in e[1]] for e in s1.output_logprobs] == [[i for i, _ in e[1]] for e in sa[1].output_logprobs]

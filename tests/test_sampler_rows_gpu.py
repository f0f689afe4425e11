"""ops.sample at a 128-row decode batch over Llama-3's vocabulary (the sampler takes any row
count; the decode fast path now reaches 128 rows): greedy is the per-row argmax, top-k = 1 with a
temperature is greedy, and the draw is a function of the RNG state."""
import pytest
import torch

from k8s_llm_monitor_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, V = 128, 128256


@pytest.fixture(scope="module")
def logits():
    ops.native()
    g = torch.Generator(device=DEV).manual_seed(11)
    return torch.randn(B, V, device=DEV, generator=g) * 1.3  # fp32: no ties for the argmax


def test_sample_greedy_128_rows(logits):
    ref = torch.argmax(logits, dim=-1).to(torch.int32)
    assert torch.equal(ops.sample(logits), ref)
    assert torch.equal(ops.sample(logits, torch.zeros(B, device=DEV)), ref)
    lb = logits.to(torch.bfloat16)
    lb[torch.arange(B, device=DEV), (torch.arange(B, device=DEV) * 1009) % V] = 64.0  # a unique bf16 maximum per row
    assert torch.equal(ops.sample(lb), torch.argmax(lb.float(), dim=-1).to(torch.int32))


def test_sample_top1_is_greedy_128_rows(logits):
    temps = torch.full((B,), 0.8, device=DEV)
    rng = torch.tensor([99, 7], device=DEV, dtype=torch.int64)
    tok = ops.sample(logits, temps, torch.ones(B, device=DEV, dtype=torch.int32), None, rng)
    assert torch.equal(tok, torch.argmax(logits, dim=-1).to(torch.int32))


def test_sample_same_rng_same_tokens_128_rows(logits):
    temps = torch.full((B,), 1.0, device=DEV)
    rng = torch.tensor([1234, 5], device=DEV, dtype=torch.int64)
    a = ops.sample(logits, temps, None, None, rng.clone())
    b = ops.sample(logits, temps, None, None, rng.clone())
    assert a.shape == (B,) and torch.equal(a, b)
    assert int(a.min()) >= 0 and int(a.max()) < V
    rng[1] = 6
    c = ops.sample(logits, temps, None, None, rng)
    assert not torch.equal(a, c), "another counter draws other tokens"

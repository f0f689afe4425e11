"""fp8 and mxfp4 MoE expert stacks on the decode path, CPU side: the picks of
ops.dec_grouped_q_config, the CPU form of ops.dec_gemm_grouped_q, the model's two-copy layout
(bf16 stacks = the dequantised codes, 5-d code and scale stacks beside them) and TP = 2 over gloo."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.models import AttnMeta, CausalLM, get_config
from k8s_llm_monitor_amd.models.checkpoint import load_checkpoint, save_checkpoint
from k8s_llm_monitor_amd.parallel.state import ParallelState

ENCS = ("fp8", "mxfp4")
KW = {"fp8": dict(f8=True), "mxfp4": dict(f4=True)}
EXPERT_KEYS = ("w13", "w2")


# ------------------------------------------------------------------ picks

# Mixtral-8x7B (F = 14336, d = 4096): (encoding, projection) -> pick at 2 / 3 / 4 / 8 local experts
MIXTRAL_PICKS = {
    ("fp8", "gate_up"): (1, 1, 8, 16),
    ("fp8", "down"): (1, 1, 8, 8),
    ("mxfp4", "gate_up"): (1, 1, 7, 8),
    ("mxfp4", "down"): (1, 1, 8, 8),
}
SHAPES = {"gate_up": (2 * 14336, 4096, ops.DEC_SWIGLU8), "down": (4096, 14336, ops.DEC_SLAB)}
TINY = {"gate_up": (2 * 1024, 512, ops.DEC_SWIGLU8), "down": (512, 1024, ops.DEC_SLAB)}  # mixtral-tiny-d128, E = 4


def _pick_ok(cfg, N, K, epi, enc):
    assert cfg[0] == 1, "the expert slabs are the split"
    for rows, ok in ((1, True), (64, True), (65, False)):
        assert ops.dec_grouped_q_form_ok(epi, cfg, rows, K=K, **KW[enc]) is ok, (cfg, rows)


@pytest.mark.parametrize("E", (2, 3, 4, 8))
@pytest.mark.parametrize("enc", ENCS)
def test_mixtral_picks(enc, E):
    for proj, (N, K, epi) in SHAPES.items():
        cfg = ops.dec_grouped_q_config(N, K, epi, E, **KW[enc])
        assert cfg == MIXTRAL_PICKS[(enc, proj)], (enc, proj, E, cfg)
        _pick_ok(cfg, N, K, epi, enc)
    # where the restriction changed the pick: bf16 takes forms the encodings do not have
    assert ops.dec_config(*SHAPES["gate_up"], experts=E) == (1, 1, 8, 16)
    assert ops.dec_config(*SHAPES["down"], experts=E) == ((1, 1, 4, 16) if E in (3, 4) else (1, 1, 8, 8))


@pytest.mark.parametrize("enc", ENCS)
def test_tiny_picks_are_the_bf16_picks(enc):
    for proj, want in (("gate_up", (1, 1, 7, 8)), ("down", (1, 1, 8, 8))):
        N, K, epi = TINY[proj]
        cfg = ops.dec_grouped_q_config(N, K, epi, 4, **KW[enc])
        assert cfg == want == ops.dec_config(N, K, epi, experts=4), (enc, proj, cfg)
        _pick_ok(cfg, N, K, epi, enc)


def test_existing_answers_are_unchanged():
    assert ops.dec_config(4096, 14336, 0, experts=8, f8=True) is None
    assert ops.dec_config(4096, 14336, 0, experts=8, f4=True) is None
    assert ops.dec_form_ok(0, (1, 1, 8, 8), 16, grouped=True, f8=True) is False
    assert ops.dec_form_ok(0, (1, 1, 8, 8), 16, grouped=True, f4=True) is False
    with pytest.raises(ValueError, match="no mxfp4 form"):
        ops.dec_gemm_grouped(torch.zeros(1, 16, 64, 8), torch.zeros(2, 4, 4, 64, 16, dtype=torch.uint8), 0, 1)


def test_config_refuses_what_cannot_launch():
    assert ops.dec_grouped_q_config(4096, 14336, 0, 8) is None, "an encoding must be named"
    assert ops.dec_grouped_q_config(4096, 14336, 0, 8, f8=True, f4=True) is None
    assert ops.dec_grouped_q_config(4096, 14336, ops.DEC_BF16, 8, f8=True) is None, "no grouped LM head"
    assert ops.dec_grouped_q_config(512, 1024 + 32, 0, 4, f8=True) is None, "fp8: K a multiple of 64"
    assert ops.dec_grouped_q_config(512, 1024 + 128, 0, 4, f4=True) is None, "mxfp4: whole 256-deep slices"
    assert not ops.dec_grouped_q_form_ok(0, (1, 1, 4, 16), 16, f8=True), "a bf16-only form"
    assert not ops.dec_grouped_q_form_ok(2, (1, 1, 8, 16), 16, f4=True), "a form without mxfp4 instantiations"
    assert not ops.dec_grouped_q_form_ok(0, (1, 1, 8, 8), 16, f4=True, K=1024 + 128)


def test_routing_table_sends_a_shape_to_bf16(monkeypatch):
    key = (512, 1024, 0, 4, "fp8")
    monkeypatch.setitem(ops.DEC_TABLE_GROUPED_Q, key, None)
    assert ops.dec_grouped_q_config(512, 1024, 0, 4, f8=True) is None
    assert ops.dec_grouped_q_config(512, 1024, 0, 4, f4=True) == (1, 1, 8, 8)
    m = CausalLM(get_config("mixtral-tiny-d128"), device="cpu", dec_weights="fp8")
    enc = m.decode_encodings()
    assert enc["w13"] == enc["w2"] == "bf16" and enc["wo"] == "fp8", "both expert projections or neither"
    assert "w13_q" not in m.layers[0] and "w2_q" not in m.layers[0]


# ------------------------------------------------------------------ CPU launch

def _stacks(E, N, K, enc, il, seed):
    """(packed bf16 stack of the dequantised weights, code stack, scale stack)."""
    g = torch.Generator().manual_seed(seed)
    wps, qps, sps = [], [], []
    for e in range(E):
        w = (torch.randn(N, K, generator=g) * 0.02 * torch.exp2(((torch.arange(N) + 3 * e) % 7 - 3).float())[:, None])
        w = w.to(torch.bfloat16)
        w = ops.interleave_gate_up8(w) if il else w
        if enc == "fp8":
            q, s = ops.quantize_rows_fp8(w)
            dq, qp, sp = ops.dequantize_rows_fp8(q, s), ops.pack_skinny_f8(q), s
        else:
            q, s = ops.quantize_mxfp4(w)
            dq = ops.dequantize_mxfp4(q, s)
            qp, sp = ops.pack_skinny_f4(q, s)
        wps.append(ops.pack_skinny(dq))
        qps.append(qp)
        sps.append(sp)
    return torch.stack(wps), torch.stack(qps), torch.stack(sps)


@pytest.mark.parametrize("M", (1, 23, 64))
@pytest.mark.parametrize("enc", ENCS)
def test_cpu_launch_equals_bf16_grouped_over_dequantised(enc, M):
    E = 3
    g = torch.Generator().manual_seed(M)
    row_w = torch.rand(M, E, generator=g) + 0.25
    row_w[torch.arange(M), torch.arange(M) % E] = 0.0
    # gate_up: A shared, SwiGLU output per expert
    N, K = 512, 512
    wp, qp, sp = _stacks(E, N, K, enc, True, 1)
    a = ops.pack_activation(torch.randn(M, K, generator=g).to(torch.bfloat16))
    shape = (E, -(-M // 16), N // 64, 64, 8)
    yq, yb = torch.zeros(shape, dtype=torch.bfloat16), torch.ones(shape, dtype=torch.bfloat16)
    assert ops.dec_gemm_grouped_q(a, qp, sp, 2, M, out=yq) == 1
    ops.dec_gemm_grouped(a, wp, 2, M, out=yb, cfg=ops.dec_grouped_q_config(N, K, 2, E, **KW[enc]))
    assert torch.equal(yq, yb)
    # down: A per expert, slabs scaled by the routing weights (zeros included)
    N, K = 256, 1024
    wp, qp, sp = _stacks(E, N, K, enc, False, 2)
    a = torch.stack([ops.pack_activation(torch.randn(M, K, generator=g).to(torch.bfloat16)) for _ in range(E)])
    for cfg in (None, (2, 1, 8, 8)):
        S = 1 if cfg is None else cfg[0]
        wq_, wb_ = torch.full((E * S * M * N,), 7.0), torch.full((E * S * M * N,), -7.0)
        assert ops.dec_gemm_grouped_q(a, qp, sp, 0, M, workspace=wq_, row_w=row_w, cfg=cfg) == E * S
        bcfg = cfg or ops.dec_grouped_q_config(N, K, 0, E, **KW[enc])
        assert ops.dec_gemm_grouped(a, wp, 0, M, workspace=wb_, row_w=row_w, cfg=bcfg) == E * S
        assert torch.equal(wq_, wb_)
        skipped = wq_.view(E, S, M, N)[torch.arange(M) % E, :, torch.arange(M)]
        assert torch.equal(skipped, torch.zeros_like(skipped)), "a zero routing weight zeroes the row's slab"


def test_cpu_launch_checks_its_arguments():
    E, N, K = 2, 256, 512
    _, qp, sp = _stacks(E, N, K, "fp8", False, 3)
    a = torch.stack([ops.pack_activation(torch.zeros(1, K, dtype=torch.bfloat16))] * E)
    ws = torch.zeros(E * 65 * N)
    with pytest.raises(ValueError, match="needs its scales"):
        ops.dec_gemm_grouped_q(a, qp, sp[:1], 0, 1, workspace=ws)
    with pytest.raises(ValueError, match="at most 64 rows"):
        ops.dec_gemm_grouped_q(a, qp, sp, 0, 65, workspace=ws)
    with pytest.raises(ValueError, match="quantised expert stack"):
        ops.dec_gemm_grouped_q(a, qp[0], sp[0], 0, 1, workspace=ws)
    with pytest.raises(ValueError, match="only the slab and SwiGLU"):
        ops.dec_gemm_grouped_q(a, qp, sp, 1, 1, workspace=ws)
    assert ops.is_mxfp4(torch.zeros(2, 1, 1, 64, 16, dtype=torch.uint8)) and not ops.is_fp8(qp.view(torch.uint8))


# ------------------------------------------------------------------ model

def _model(enc, seed=3):
    return CausalLM(get_config("mixtral-tiny-d128"), device="cpu", seed=seed, pstate=ParallelState(), dec_weights=enc)


@pytest.fixture(scope="module")
def models():
    return {enc: _model(enc) for enc in ("bf16",) + ENCS}


def _dq_stack(L, key, dtype):
    """The dequantised values of the code stack, [E, out, in] in the packed copy's row order."""
    q, s = L[key + "_q"], L[key + "_qs"]
    if ops.is_fp8(q):
        return torch.stack([ops.dequantize_rows_fp8(ops.unpack_skinny_f8(q[e]), s[e], dtype) for e in range(q.shape[0])])
    return torch.stack([ops.dequantize_mxfp4(*ops.unpack_skinny_f4(q[e], s[e]), dtype) for e in range(q.shape[0])])


def _decode_logits(m):
    """Prefill two prompts into a paged cache, then one decode step of both: its logits."""
    bs, nb = 16, 8
    g = torch.Generator().manual_seed(0)
    kv = [(torch.randn(nb, m.hkv, m.D // 8, bs, 8, generator=g).to(m.dtype),
           torch.randn(nb, m.hkv, m.D, bs, generator=g).to(m.dtype)) for _ in m.layers]
    T = torch.tensor([5, 9])
    ids = torch.randint(0, m.cfg.vocab_size, (14,), generator=torch.Generator().manual_seed(1), dtype=torch.int32)
    pos = torch.cat([torch.arange(5), torch.arange(9)]).to(torch.int32)
    slots = torch.cat([torch.arange(5), 16 + torch.arange(9)]).to(torch.int32)
    meta = AttnMeta(is_prefill=True, positions=pos, slot_mapping=slots, cu_seqlens=torch.tensor([0, 5, 14], dtype=torch.int32),
                    logits_idx=torch.tensor([4, 13]))
    pre = m.forward(ids, meta, kv)
    lens = T + 1
    dm = AttnMeta(is_prefill=False, positions=(lens - 1).to(torch.int32), slot_mapping=torch.tensor([5, 25], dtype=torch.int32),
                  block_tables=torch.tensor([[0, 3], [1, 2]], dtype=torch.int32), seq_lens=lens.to(torch.int32))
    return pre, m.forward(torch.tensor([7, 99], dtype=torch.int32), dm, kv)


@pytest.mark.parametrize("enc", ENCS)
def test_model_holds_code_stacks_beside_the_dequantised_bf16_stacks(models, enc):
    m, plain = models[enc], models["bf16"]
    E = m.cfg.n_experts
    de = m.decode_encodings()
    assert de["w13"] == de["w2"] == enc, de
    assert set(de.values()) == {enc}
    assert plain.decode_encodings()["w13"] == plain.decode_encodings()["w2"] == "bf16"
    extra = 0
    for L in m.layers:
        for key in EXPERT_KEYS:
            q, s = L[key + "_q"], L[key + "_qs"]
            assert q.dim() == 5 and q.shape[0] == E and tuple(q.shape[3:]) == (64, 16)
            assert (ops.is_fp8(q) if enc == "fp8" else ops.is_mxfp4(q)) and s.shape[0] == E
            out, inn = L[key + "_dg"].shape[1] * 16, L[key + "_dg"].shape[2] * 32
            assert ops.grouped_q_wdims(q) == (E, out, inn)
            assert tuple(s.shape) == ((E, out) if enc == "fp8" else (E, out // 16, inn // 128, 16, 4))
            # the bf16 stacks are exactly the dequantised codes
            dq = _dq_stack(L, key, m.dtype)
            assert torch.equal(torch.stack([ops.unpack_skinny(w) for w in L[key + "_dg"]]), dq), key
            canon = m.canonical(L, key)
            want = torch.stack([ops.deinterleave_gate_up8(w) for w in dq]) if key == "w13" else dq
            assert torch.equal(canon, want), key
            # and requantising them reproduces the codes and scales
            for e in range(E):
                if enc == "fp8":
                    q2, s2 = ops.quantize_rows_fp8(dq[e])
                    assert torch.equal(ops.pack_skinny_f8(q2).view(torch.uint8), q[e].view(torch.uint8)), (key, e)
                    assert torch.equal(s2, s[e]), (key, e)
                else:
                    q2, s2 = ops.pack_skinny_f4(*ops.quantize_mxfp4(dq[e]))
                    assert torch.equal(q2, q[e]) and torch.equal(s2, s[e]), (key, e)
            extra += q.numel() * q.element_size() + s.numel() * s.element_size()
    dense = sum(L[k + sfx].numel() * L[k + sfx].element_size() for L in m.layers for k in ("wqkv", "wo")
                for sfx in ("_q", "_qs"))
    head = sum(t.numel() * t.element_size() for t in (m.lm_head_q, m.lm_head_qs))
    assert m.num_local_params() == plain.num_local_params()
    assert m.resident_weight_bytes() == plain.resident_weight_bytes() + extra + dense + head
    assert extra > dense + head, "the expert stacks are most of the model"


@pytest.mark.parametrize("enc", ENCS)
def test_decode_runs_the_quantised_grouped_launch_and_matches_bf16_decoding(models, enc, monkeypatch):
    m = models[enc]
    other = _model("bf16", seed=9)
    other.copy_weights_from(m)
    assert not any(k.endswith("_q") for k in other.layers[0])
    seen = []
    real = ops.dec_gemm_grouped_q

    def spy(a, wq, wqs, epi, rows, **kw):
        seen.append((epi, rows, enc if (ops.is_fp8(wq) if enc == "fp8" else ops.is_mxfp4(wq)) else "?"))
        return real(a, wq, wqs, epi, rows, **kw)

    monkeypatch.setattr(ops, "dec_gemm_grouped_q", spy)
    pre_q, dec_q = _decode_logits(m)
    assert sorted(set(seen)) == [(0, 2, enc), (2, 2, enc)], seen
    assert len(seen) == 2 * len(m.layers)
    n = len(seen)
    pre_b, dec_b = _decode_logits(other)
    assert len(seen) == n, "the bf16-decoding model launches no quantised GEMM"
    assert torch.equal(pre_q, pre_b), "prefill reads the dequantised stacks"
    assert torch.equal(dec_q, dec_b), "one model, two encodings: the same decode logits"


@pytest.mark.parametrize("enc", ENCS)
def test_checkpoint_round_trip_and_requantisation(models, enc, tmp_path):
    m = models[enc]
    _, want = _decode_logits(m)
    save_checkpoint(m, tmp_path / "ckpt")
    third = _model(enc, seed=11)
    assert not torch.equal(third.layers[0]["w13_q"].view(torch.uint8), m.layers[0]["w13_q"].view(torch.uint8))
    load_checkpoint(third, tmp_path / "ckpt")
    for La, Lb in zip(m.layers, third.layers):
        for key in EXPERT_KEYS:
            assert torch.equal(Lb[key + "_q"].view(torch.uint8), La[key + "_q"].view(torch.uint8)), key
            assert torch.equal(Lb[key + "_qs"], La[key + "_qs"]), key
            assert torch.equal(third.canonical(Lb, key), m.canonical(La, key)), key
    assert torch.equal(_decode_logits(third)[1], want)
    # a weight copy into a quantised model requantises; a second _init_skinny reproduces the codes
    src = _model("bf16", seed=9)
    third.copy_weights_from(src)
    L = third.layers[0]
    assert torch.equal(torch.stack([ops.unpack_skinny(w) for w in L["w2_dg"]]), _dq_stack(L, "w2", third.dtype))
    assert not torch.equal(third.canonical(L, "w2"), m.canonical(m.layers[0], "w2"))
    q0, s0 = L["w13_q"].clone(), L["w13_qs"].clone()
    third._init_skinny()
    L = third.layers[0]
    assert torch.equal(L["w13_q"].view(torch.uint8), q0.view(torch.uint8)) and torch.equal(L["w13_qs"], s0)
    third.begin_load()
    assert not any(k.endswith(("_q", "_qs")) for k in third.layers[0]), "_drop_derived drops the stacks' codes"


def test_one_layout_packed_stacks_take_the_dequantised_values(monkeypatch):
    """The GPU's single packed copy (forced on the CPU): L[key] is the packed bf16 stack, the codes beside it."""
    monkeypatch.setattr(CausalLM, "ONE_LAYOUT", "force")
    m = _model("fp8")
    assert m._packed
    L = m.layers[0]
    for key in EXPERT_KEYS:
        assert L[key] is L[key + "_dg"] and key + "_pg" not in L
        assert torch.equal(torch.stack([ops.unpack_skinny(w) for w in L[key]]), _dq_stack(L, key, m.dtype))
    other = _model("bf16", seed=9)
    other.copy_weights_from(m)
    assert other._packed and "w13_q" not in other.layers[0]
    for a, b in zip(_decode_logits(m), _decode_logits(other)):
        assert torch.equal(a, b)


def test_log_line_only_where_the_stacks_stay_bf16(monkeypatch, caplog):
    import logging

    with caplog.at_level(logging.INFO, logger="k8s_llm_monitor_amd.models.llama"):
        _model("fp8")
    assert "leaves the MoE expert stacks on bf16" not in caplog.text
    caplog.clear()
    monkeypatch.setitem(ops.DEC_TABLE_GROUPED_Q, (2048, 512, 2, 4, "fp8"), None)
    with caplog.at_level(logging.INFO, logger="k8s_llm_monitor_amd.models.llama"):
        _model("fp8")
    assert "leaves the MoE expert stacks on bf16 (no fp8 grouped form" in caplog.text


# ------------------------------------------------------------------ TP = 2 over gloo

def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_worker(rank, world, port, model, one_layout, moe_decode, ckpt, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank), K8SLLM_MOE_DECODE=moe_decode)
    torch.set_num_threads(2)
    from k8s_llm_monitor_amd.parallel.state import destroy, init_parallel

    if one_layout:  # the GPU's packed expert stacks: the EP all-to-all decode on the shared-A grouped GEMM too
        CausalLM.ONE_LAYOUT = "force"
    try:
        ps = init_parallel(tp_size=world, device="cpu")
        cfg = get_config(model)
        ref = CausalLM(cfg, device="cpu", dtype=torch.float32, seed=11, pstate=ParallelState(), dec_weights="fp8")
        # The TP model takes the TP = 1 model's (dequantised) weights: a row-parallel shard of wo
        # quantises on a finer or equal row scale, which holds every code of the shard exactly,
        # and experts are sharded whole - so both models hold the same values.
        path = os.path.join(ckpt, f"rank{rank}")
        save_checkpoint(ref, path)
        tpm = CausalLM(cfg, device="cpu", dtype=torch.float32, seed=12, pstate=ps, dec_weights="fp8")
        load_checkpoint(tpm, path, strict=False)  # the other rank's experts stay unread
        assert tpm._packed == one_layout and tpm.moe_decode == moe_decode
        lo, hi = tpm.e_lo, tpm.e_hi
        same = all(torch.equal(Lt[k + "_q"].view(torch.uint8), Lr[k + "_q"][lo:hi].view(torch.uint8))
                   and torch.equal(Lt[k + "_qs"], Lr[k + "_qs"][lo:hi])
                   for Lt, Lr in zip(tpm.layers, ref.layers) for k in EXPERT_KEYS)
        seen = []
        real = ops.dec_gemm_grouped_q

        def spy(a, wq, wqs, epi, rows, **kw):
            seen.append((epi, wq.shape[0], ops.is_fp8(wq)))
            return real(a, wq, wqs, epi, rows, **kw)

        ops.dec_gemm_grouped_q = spy
        _, a = _decode_logits(tpm)
        mine = sorted(set(seen))
        seen.clear()
        _, b = _decode_logits(ref)
        q.put((rank, (a - b).abs().max().item(), tpm.decode_encodings(), same, mine))
        destroy()
    except Exception as e:  # noqa: BLE001
        import traceback

        q.put((rank, repr(e) + traceback.format_exc(), None, None, None))


@pytest.mark.parametrize("model,one_layout,moe_decode", [
    ("mixtral-tiny", False, "allreduce"), ("mixtral-tiny", False, "a2a"),
    # packed stacks: the all-to-all form launches over the codes as well (row-major stacks keep gemm_skinny there)
    ("mixtral-tiny-d128", True, "a2a")])
def test_tp2_fp8_experts_match_tp1(model, one_layout, moe_decode, tmp_path):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_tp_worker, args=(r, world, port, model, one_layout, moe_decode, str(tmp_path), q))
             for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(60)
    launches = [(0, 2, True), (2, 2, True)] if one_layout or moe_decode == "allreduce" else []
    for rank, err, enc, same, seen in res:
        assert not isinstance(err, str), err
        assert enc["w13"] == enc["w2"] == "fp8", f"rank {rank}: {enc}"
        assert same, f"rank {rank}: its codes are not the TP = 1 model's codes of its experts"
        assert seen == launches, f"rank {rank}: quantised grouped launches over 2 local experts, {seen}"
        assert err < 2e-3, f"rank {rank}: max |tp - ref| = {err}"

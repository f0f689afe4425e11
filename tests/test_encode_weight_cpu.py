"""ops.encode_weight, the one owner of "encode a decode projection": quantise, dequantise, the
[8 gate | 8 up] row permutation of codes and scales, pack.  fp8 and mxfp4, with and without
``gate_up8`` and ``settle``, on a [64, 256] bf16 weight with a row of zeros, a row whose amax sits on
the fp8 scale boundary (448 * 2^-8) and a row whose every block's amax sits on the mxfp4 one
(6 * 2^-3), where the first-pass and the settled scale differ or tie."""
import pytest
import torch

from k8s_llm_monitor_amd import ops


def _weight():
    g = torch.Generator().manual_seed(11)
    w = torch.randn(64, 256, generator=g) * 0.05
    w = w * torch.exp2((torch.arange(64) % 5 - 2).float())[:, None]
    w[3] = 0.0
    w[5] = w[5].clamp(-1.0, 1.0)
    w[5, 77] = 448.0 / 256  # amax / 448 = 2^-8 exactly
    w[6] = w[6].clamp(-0.5, 0.5)
    w[6, ::32] = 0.75  # every block's amax / 6 = 2^-3 exactly
    w[7, ::32] = -0.47  # rounds up to 0.5 * 2^0 = the top of a coarser block scale than 0.47 asks for
    return w.to(torch.bfloat16)


def _decode(enc, qp, sp, gate_up8):
    if enc == "fp8":
        v = ops.dequantize_rows_fp8(ops.unpack_skinny_f8(qp), sp)
    else:
        v = ops.dequantize_mxfp4(*ops.unpack_skinny_f4(qp, sp))
    return ops.deinterleave_gate_up8(v) if gate_up8 else v


@pytest.mark.parametrize("gate_up8", [False, True])
@pytest.mark.parametrize("enc", ["fp8", "mxfp4"])
def test_codes_decode_to_the_returned_values_and_settle(enc, gate_up8):
    w = _weight()
    first = ops.encode_weight(w, enc, gate_up8)
    settled = ops.encode_weight(w, enc, gate_up8, settle=True)
    for deq, qp, sp in (first, settled):
        assert deq.dtype == w.dtype and deq.shape == w.shape
        assert qp.shape == ((4, 4, 64, 16) if enc == "fp8" else (4, 2, 64, 16))
        assert (sp.shape, sp.dtype) == (((64,), torch.float32) if enc == "fp8" else ((4, 2, 16, 4), torch.uint8))
        assert torch.equal(_decode(enc, qp, sp, gate_up8), deq), "codes x scales are exactly the returned values"
    assert torch.equal(first[0], settled[0]), "settling changes codes and scales, never a value"
    # the zero row stays zero; the encoding's own boundary row keeps its amax exactly (the top code)
    assert not first[0][3].any()
    assert (first[0][5].abs().max() == 1.75) if enc == "fp8" else (first[0][6].abs().max() == 0.75)
    # re-encoding the values reproduces the settled codes byte for byte, settling again or not
    for again in (ops.encode_weight(settled[0], enc, gate_up8, settle=True), ops.encode_weight(settled[0], enc, gate_up8)):
        assert torch.equal(again[0], settled[0])
        assert torch.equal(again[1].view(torch.uint8), settled[1].view(torch.uint8))
        assert torch.equal(again[2].view(torch.uint8), settled[2].view(torch.uint8))
    # the row permutation is of codes and scales alike: gate_up8 output = the plain output's rows interleaved
    if gate_up8:
        plain = ops.encode_weight(w, enc, False, settle=True)
        assert torch.equal(_decode(enc, settled[1], settled[2], False), ops.interleave_gate_up8(plain[0]))


def test_unknown_encoding_and_enc_kw():
    with pytest.raises(ValueError):
        ops.encode_weight(_weight(), "int4")
    _, q8, _ = ops.encode_weight(_weight(), "fp8")
    _, q4, _ = ops.encode_weight(_weight(), "mxfp4")
    assert ops.enc_kw("fp8") == ops.enc_kw(q8) == {"f8": True}
    assert ops.enc_kw("mxfp4") == ops.enc_kw(q4) == ops.enc_kw(q4[None]) == {"f4": True}
    with pytest.raises(ValueError):
        ops.enc_kw("bf16")

"""Constrained decoding on the CPU: the guide compiler against Python's ``re`` and ``json``, the
mask reference against a naive walk, the guided CPU sampler against the sampler over -inf
prefilled logits, the vocabulary bytes of both tokenizers, and the CPU engine end to end.

``\\d \\w \\s`` are the ASCII classes, so the yardstick is ``re.compile(p, re.ASCII)``; strings are
compared through their UTF-8 bytes, and bytes that are not UTF-8 must be rejected."""
import json
import pickle
import random
import re
import time
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from k8s_llm_monitor_amd import ops
from k8s_llm_monitor_amd.engine import EngineConfig, EngineService, LLMEngine, SamplingParams
from k8s_llm_monitor_amd.engine.guide import Guide, compile_guide
from k8s_llm_monitor_amd.engine.tokenizer import HFTokenizer, tokenizer_for, vocab_bytes
from k8s_llm_monitor_amd.models.config import get_config
from k8s_llm_monitor_amd.ops import reference as ref

# every construct of the subset; all inside it (none may be skipped)
PATTERNS = [
    r"abc", r"a|b|cd", r"(ab)*c", r"(?:ab)+", r"a?b", r"\d{3}-\d{4}", r"[a-z]{2,4}", r"[^a-c]x", r".+",
    r"\w+@\w+\.com", r"\s*\S+", r"\D\W", r"é+", r"[α-ω]{1,3}", r"[^é]", r"\x41é", r"a{2,}", r"^abc$",
    r"\.\*\\", r"[\]\-a]+", r"[]a]", r"(a|b){3}(c|)", r"x{0}y", r"日本|中国", r".", r"[\d\s]+", r"[^\n\d]*",
    r"\t\n\r", r"é日", r"[一-鿿]+", r"(low|medium|high)", r"pod-[a-z0-9]{1,5}(-[a-z0-9]+)?",
    r"-?(0|[1-9]\d*)(\.\d+)?", r"[^\W\d]+", r"[\w.-]+", r"a{3}b{0,2}", r"(?:x|yz){2,3}", r"\$\^\(\)\[\]\{\}\|\?\+",
    r"[^\x00-\x7f]", r"[a-c\d]*z", r"\S\s\S", r"(é|e)(😀|!)?", r"(?:a{1}){2}", r"[.][*]", r"()a(|b)", r"\W{2}",
    r"x{2,3}|y", r"{a}", r"a{0,2}x", r"[^\s\w]",
]
UNSUPPORTED = [r"(a)\1", r"(?=a)b", r"(?!a)b", r"(?<=a)b", r"a*?", r"a+?", r"a??", r"a{1,2}?", r"(?i)a", r"a^b",
               r"a$b", r"(?P<n>a)", r"a++", r"\bfoo", r"\Afoo", r"foo\Z", r"[a", r"(a", r"a)", r"*a", "a\\",
               r"[[:alpha:]]", r"\p{L}", r"a{3,2}"]
ALPHABET = "abcxyz019 .-@\n\t_\\*]!é日α中😀"


def random_walk(g: Guide, rng: random.Random, stop: float = 0.25, limit: int = 300):
    """Bytes of a random accepting walk (None if the limit came first)."""
    s, out = 0, bytearray()
    for _ in range(limit):
        nxt = np.flatnonzero(g.trans[s] >= 0)
        if g.accept[s] and (len(nxt) == 0 or rng.random() < stop):
            return bytes(out)
        b = int(nxt[rng.randrange(len(nxt))])
        out.append(b)
        s = int(g.trans[s, b])
    return bytes(out) if g.accept[s] else None


def re_accepts(rx, data: bytes) -> bool:
    try:
        return rx.fullmatch(data.decode("utf-8")) is not None
    except UnicodeDecodeError:
        return False  # never a lone continuation byte, an overlong form or a surrogate


def check_dfa(g: Guide):
    n = g.n
    assert g.trans.shape == (n, 256) and g.accept.shape == (n,) and g.trans.max() < n and g.trans.min() >= -1
    live = g.accept.copy()
    for _ in range(n):  # every state reaches an accepting one
        live |= np.concatenate([live, [False]])[g.trans].any(axis=1)
    assert live.all()
    seen, todo = {0}, [0]
    while todo:  # ... and is reached from state 0
        for t in set(g.trans[todo.pop()].tolist()) - {-1}:
            if t not in seen:
                seen.add(t)
                todo.append(t)
    assert len(seen) == n


def test_pattern_list():
    assert len(PATTERNS) >= 40 and len(set(PATTERNS)) == len(PATTERNS)


@pytest.mark.parametrize("pat", PATTERNS)
def test_regex_matches_python_re(pat):
    rng = random.Random(PATTERNS.index(pat))
    g = compile_guide({"regex": pat})
    rx = re.compile(pat, re.ASCII)
    check_dfa(g)
    walks = [w for w in (random_walk(g, rng) for _ in range(60)) if w is not None]
    assert walks
    for w in walks:
        assert rx.fullmatch(w.decode("utf-8")) is not None, (pat, w)
        assert g.matches(w)
    cands = ["".join(rng.choice(ALPHABET) for _ in range(rng.randint(0, 6))).encode() for _ in range(300)]
    for w in walks[:30]:  # one-byte mutations of accepted strings: replaced, dropped, inserted
        w = bytearray(w)
        i = rng.randrange(len(w) + 1)
        b = rng.choice([rng.randrange(256), ord(rng.choice("abz09 -\n")), 0x80, 0xC3, 0xE6])
        kind = rng.randrange(3)
        if kind == 0 and i < len(w):
            w[i] = b
        elif kind == 1 and i < len(w):
            del w[i]
        else:
            w.insert(i, b)
        cands.append(bytes(w))
    for c in cands:
        assert g.matches(c) == re_accepts(rx, c), (pat, c)


@pytest.mark.parametrize("pat", UNSUPPORTED)
def test_unsupported_regex_raises(pat):
    with pytest.raises(ValueError):
        compile_guide({"regex": pat})


def test_specs_are_plain_data_and_cached():
    spec = {"regex": r"[a-f]{4}"}
    g = compile_guide(spec)
    assert compile_guide(pickle.loads(pickle.dumps(spec))) is g  # cached by canonical text
    assert compile_guide({"choice": ["b", "a"]}).key != compile_guide({"choice": ["a", "b"]}).key
    g = compile_guide({"choice": ["low", "medium", "high", "日本"]})
    assert all(g.matches(c) for c in ("low", "medium", "high", "日本")) and not g.matches("lo") and not g.matches("")
    for bad in (None, {}, {"choice": []}, {"choice": ["a", 1]}, {"regex": 5}, {"json_schema": []}, {"grammar": "x"},
                {"choice": ["a"], "regex": "a"}, {"json_schema": {"type": "json_object"}}, {"json_schema": {}}):
        with pytest.raises(ValueError):
            compile_guide(bad)
    with pytest.raises(ValueError, match="schema is needed"):
        compile_guide({"json_schema": {"type": "json_object"}})
    with pytest.raises(ValueError, match="matches nothing"):
        compile_guide({"regex": r"a[^\S\s]"})


def test_state_limit_and_hostile_repeat():
    assert compile_guide({"regex": "[ab]{511}"}).n == 512
    with pytest.raises(ValueError, match="guide_max_states|too large"):
        compile_guide({"regex": "[ab]{512}"})
    assert compile_guide({"regex": "[ab]{40}"}, max_states=41).n == 41
    with pytest.raises(ValueError):
        compile_guide({"regex": "[ab]{41}"}, max_states=41)
    for hostile in ("[a-z]{5000}", "(a{1000}){1000}", "(a|b)*a(a|b){24}", ".{0,3000}"):
        t0 = time.perf_counter()
        with pytest.raises(ValueError):
            compile_guide({"regex": hostile})
        assert time.perf_counter() - t0 < 0.5, hostile


# ------------------------------------------------------------------------------------------ schema

SCHEMA = {"type": "object", "title": "finding", "properties": {
    "severity": {"enum": ["low", "medium", "high"]},
    "pod": {"type": "string", "minLength": 1, "maxLength": 6},
    "restarts": {"type": "integer"},
    "score": {"type": "number"},
    "ready": {"type": "boolean"},
    "owner": {"type": "null"},
    "kind": {"const": "pod"},
    "ports": {"type": "array", "items": {"type": "integer"}, "minItems": 1, "maxItems": 3},
    "tags": {"type": "array", "items": {"type": "string", "maxLength": 2}},
    "inner": {"type": "object", "properties": {"ok": {"type": "boolean"}, "n": {"enum": [1, 2.5, None, True, "x"]}}},
}, "required": ["severity"], "additionalProperties": False}


def test_schema_walks_parse_with_declared_types():
    g = compile_guide({"json_schema": SCHEMA})
    check_dfa(g)
    rng = random.Random(1)
    n = 0
    for _ in range(80):
        w = random_walk(g, rng, stop=1.0, limit=2000)
        if w is None:
            continue
        n += 1
        text = w.decode("utf-8")
        d = json.loads(text)
        assert list(d) == list(SCHEMA["properties"])  # every property, in the listed order
        assert d["severity"] in ("low", "medium", "high") and d["kind"] == "pod" and d["owner"] is None
        assert isinstance(d["pod"], str) and 1 <= len(d["pod"]) <= 6
        assert type(d["restarts"]) is int and isinstance(d["score"], (int, float)) and type(d["ready"]) is bool
        assert 1 <= len(d["ports"]) <= 3 and all(type(p) is int for p in d["ports"])
        assert all(isinstance(t, str) and len(t) <= 2 for t in d["tags"])
        assert type(d["inner"]["ok"]) is bool and d["inner"]["n"] in (1, 2.5, None, True, "x")
        assert g.matches(text)
    assert n >= 40
    ok = '{"severity":"low","pod":"a\\"\\u00e9日","restarts":-7,"score":1.5e3,"ready":true,"owner":null,' \
         '"kind":"pod","ports":[1,20],"tags":[],"inner":{"ok":false,"n":2.5}}'
    assert g.matches(ok) and json.loads(ok)["pod"] == 'a"é日'
    for bad in (ok.replace(":", ": ", 1), ok.replace('"low"', '"lower"'), ok.replace("[1,20]", "[]"),
                ok.replace("[1,20]", "[1,2,3,4]"), ok.replace("-7", "07"), ok.replace("-7", "1.0"),
                ok.replace('"tags":[]', '"tags":["abc"]'), ok.replace("true", "True"), ok[:-1], ok + " ",
                ok.replace('a\\"', "a\n"), ok.replace('"severity":"low",', "")):
        assert not g.matches(bad), bad
    big = compile_guide({"json_schema": {"type": "integer"}})
    assert big.matches("0") and big.matches("-123456789012345678") and not big.matches("1234567890123456789") \
        and not big.matches("-") and not big.matches("01")


@pytest.mark.parametrize("schema", [
    {"$ref": "#/x"}, {"anyOf": [{"type": "null"}]}, {"oneOf": []}, {"allOf": []}, {"type": "string", "pattern": "a"},
    {"type": "string", "format": "date"}, {"type": ["string", "null"]}, {"type": "integer", "minimum": 0},
    {"type": "object", "properties": {"a": {"type": "frob"}}}, {"type": "object", "patternProperties": {}},
    {"type": "array"}, {"type": "array", "items": {"type": "integer"}, "uniqueItems": True}, {"enum": [[1]]},
    {"const": {"a": 1}}, {"type": "string", "minLength": 3, "maxLength": 2}, {"properties": {}},
    {"type": "object", "properties": {"s": {"type": "string", "maxLength": 400}}},  # past the state limit
])
def test_refused_schema_keywords(schema):
    with pytest.raises(ValueError):
        compile_guide({"json_schema": schema})


# -------------------------------------------------------------------------------- masks and sampling

def small_vocab(V=300, seed=0):
    r = random.Random(seed)
    vb = [bytes([i]) for i in range(256)]
    while len(vb) < V:
        vb.append("".join(r.choice('ab01-{}":,low') for _ in range(r.randint(1, 5))).encode())
    vb[1] = vb[2] = vb[270] = b""
    vb[271] = "é".encode()[:1]  # half a character
    vb[272] = b"a" * 40
    return vb


def test_guide_mask_against_a_naive_walk():
    vb, eos = small_vocab(), (2, 299)
    for spec in ({"choice": ["low", "a-1", "é"]}, {"regex": r"[ab01]{1,45}"}, {"regex": r"(ab)*"},
                 {"json_schema": {"type": "object", "properties": {"a": {"enum": ["low", "b"]}}}}):
        g = compile_guide(spec)
        m = ref.guide_mask(g.trans, g.accept, vb, eos)
        assert m.shape == (g.n, len(vb)) and m.dtype == torch.bool
        for s in range(g.n):
            for t, b in enumerate(vb):
                if t in eos:
                    want = bool(g.accept[s])
                else:
                    cur = s
                    for byte in b:
                        cur = int(g.trans[cur, byte]) if cur >= 0 else -1
                    want = len(b) > 0 and cur >= 0
                    assert ref.guide_advance(g.trans, s, b) == (cur if b else s)
                assert bool(m[s, t]) == want, (spec, s, t)
        assert m.any(1).all()  # no empty row: every single byte is a token here


def test_cpu_sampler_with_guide_equals_prefilled_logits():
    V = 300
    vb, eos = small_vocab(V), (2, 299)
    guides = [compile_guide(s) for s in ({"choice": ["low", "a-1"]}, {"regex": r"[ab01]{3,9}"}, {"choice": ["Q"]},
                                         {"regex": "Q|R"})]
    g = torch.Generator().manual_seed(0)
    B = 12
    logits = torch.randint(-64, 65, (B, V), generator=g).float() / 8
    kinds = [(0.0, 0, 1.0), (1.0, 0, 1.0), (0.7, 5, 1.0), (1.3, 0, 0.6), (1.0, 40, 0.9), (1.0, 1, 1.0)]
    temps = torch.tensor([kinds[b % 6][0] for b in range(B)])
    top_k = torch.tensor([kinds[b % 6][1] for b in range(B)], dtype=torch.int32)
    top_p = torch.tensor([kinds[b % 6][2] for b in range(B)])
    gs = ops.GuideState(B, V, vb, eos, "cpu", rows=sum(q.n for q in guides))
    gslots = torch.full((B,), -1, dtype=torch.int32)
    pre = logits.clone()
    local = {}
    for b in range(B):
        if b % 5 == 4:
            continue  # an unguided row
        q = guides[2 + b % 2] if b < 6 else guides[b % 2]  # rows 0..5: one or two allowed tokens, every path
        gs.reset(b, q, [])
        gslots[b] = b
        allowed = ref.guide_mask(q.trans, q.accept, vb, eos)[0]
        assert int(allowed.sum()) == (1 + b % 2 if b < 6 else int(allowed.sum()))
        pre[b] = logits[b].masked_fill(~allowed, float("-inf"))
        local[b] = q
    for step in range(3):
        rng = torch.tensor([5, step], dtype=torch.int64)
        before = gs.state.clone()
        got = ops.sample(logits, temps, top_k, top_p, rng.clone(), guide=gs, gslots=gslots)
        want = ops.sample(pre, temps, top_k, top_p, rng.clone())
        assert torch.equal(got, want)
        for b, q in local.items():
            t = int(got[b])
            assert torch.isfinite(pre[b, t])  # only finite entries are ever drawn
            rows = gs.resident_rows(q)
            s0 = int(np.flatnonzero(rows == int(before[b]))[0])
            s1 = ref.guide_advance(q.trans, s0, vb[t]) if t not in eos else s0
            assert int(gs.state[b]) == int(rows[s1])
            allowed = ref.guide_mask(q.trans, q.accept, vb, eos)[s1]
            pre[b] = logits[b].masked_fill(~allowed, float("-inf"))
    assert not torch.equal(gs.state, torch.full((B,), -1, dtype=torch.int32))


# ------------------------------------------------------------------------------------ vocabulary bytes

def test_vocab_bytes_of_the_builtin_tokenizer():
    mc = get_config("llama-tiny")
    tok = tokenizer_for(mc)
    vb = vocab_bytes(tok, mc.vocab_size)
    assert len(vb) == mc.vocab_size and vb[mc.bos_id] == b"" and all(vb[e] == b"" for e in mc.eos_ids)
    for t in range(mc.vocab_size):
        assert vb[t].decode("utf-8", errors="replace") == tok.decode([t]), t
    ids = list(range(mc.vocab_size))
    assert b"".join(vb[t] for t in ids).decode("utf-8", errors="replace") == tok.decode(ids)
    big = get_config("llama-tiny-d128")  # ids beyond the merges fold onto them, as decode does
    tb = tokenizer_for(big)
    vbig = vocab_bytes(tb, big.vocab_size)
    assert all(vbig[t].decode("utf-8", errors="replace") == tb.decode([t]) for t in range(big.vocab_size))


def test_vocab_bytes_of_a_byte_level_hf_vocabulary(tmp_path):
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers

    from k8s_llm_monitor_amd.engine.tokenizer import _gpt2_unicode_to_byte

    b2u = {b: u for u, b in _gpt2_unicode_to_byte().items()}
    raw = [bytes([i]) for i in range(256)] + [b"ab", " pod".encode(), "日".encode(), "日".encode()[:2], b"\n\n"]
    vocab = {"".join(b2u[x] for x in bs): i for i, bs in enumerate(raw)}
    assert len(vocab) == len(raw)
    tk = Tokenizer(models.BPE(vocab=vocab, merges=[]))
    tk.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False)
    tk.decoder = decoders.ByteLevel()
    tk.add_special_tokens(["<|eot|>"])
    path = tmp_path / "tokenizer.json"
    tk.save(str(path))
    tok = HFTokenizer(path, None, len(raw))
    vb = vocab_bytes(tok, len(raw) + 1)
    assert vb[: len(raw)] == raw and vb[len(raw)] == b""  # the special token has no bytes
    half = raw.index("日".encode()[:2])
    assert vb[half] == b"\xe6\x97" and tok.token_bytes(half) != vb[half]  # token_bytes gives U+FFFD
    assert (vb[half] + b"\xa5").decode() == "日"
    wp = Tokenizer(models.WordPiece(vocab={"[UNK]": 0, "pod": 1, "##s": 2}, unk_token="[UNK]"))
    wpath = tmp_path / "wp.json"
    wp.save(str(wpath))
    with pytest.raises(ValueError, match="byte-level vocabulary"):
        vocab_bytes(HFTokenizer(wpath, None, None), 3)


# ---------------------------------------------------------------------------------------------- engine

CHOICE = {"choice": ["low", "medium", "high"]}
REGEX = {"regex": r"pod-[a-z]{3}-\d{2}"}
OBJ = {"json_schema": {"type": "object", "properties": {"severity": {"enum": ["low", "high"]},
                                                        "restarts": {"type": "integer"},
                                                        "ready": {"type": "boolean"}}}}


@pytest.fixture(scope="module")
def cpu_engine():
    return LLMEngine(EngineConfig(model="llama-tiny", max_num_seqs=8, max_model_len=256, num_blocks=128,
                                  dtype="float32", seed=0), device="cpu")


def test_cpu_engine_end_to_end(cpu_engine):
    eng = cpu_engine
    st = eng.stats()
    assert st["guide_enabled"] is False and st["guide_state_bytes"] == 0 and st["guides_resident"] == 0 \
        and st["guide_slots_in_use"] == 0 and eng.runner.gd is None
    specs = [CHOICE, REGEX, OBJ, None]
    seqs = [eng.add_request(f"pod {i} restarts", SamplingParams(max_tokens=80, temperature=1.0, guide=specs[i % 4]))
            for i in range(8)]
    assert eng.stats()["guide_enabled"] and eng.stats()["guides_resident"] == 3
    used = 0
    while eng.has_work():
        eng.step()
        used = max(used, eng.stats()["guide_slots_in_use"])
    assert used == 6 and eng.stats()["guide_slots_in_use"] == 0
    for i, s in enumerate(seqs):
        text = eng.decode_text(s)
        if specs[i % 4] is None:
            continue
        assert s.finish_reason == "stop", (text, s.finish_reason)
        assert compile_guide(specs[i % 4]).matches(text), text
        if specs[i % 4] is CHOICE:
            assert text in CHOICE["choice"]
        elif specs[i % 4] is REGEX:
            assert re.fullmatch(REGEX["regex"], text)
        else:
            d = json.loads(text)
            assert list(d) == ["severity", "restarts", "ready"] and d["severity"] in ("low", "high") \
                and type(d["restarts"]) is int and type(d["ready"]) is bool
    assert eng.stats()["guide_state_bytes"] == eng.runner.gd.nbytes > 0
    assert eng.runner.memory_report()["guide_state_bytes"] == eng.runner.gd.nbytes


def test_engine_refuses_what_it_cannot_guide(cpu_engine):
    eng = cpu_engine
    with pytest.raises(ValueError, match="ignore_eos"):
        eng.add_request("x", SamplingParams(guide=CHOICE, ignore_eos=True))
    with pytest.raises(ValueError, match="look-around|not supported"):
        eng.add_request("x", SamplingParams(guide={"regex": "(?=a)a"}))
    with pytest.raises(ValueError, match="too large"):
        eng.add_request("x", SamplingParams(guide={"regex": "[ab]{600}"}))
    ps = eng.ps
    try:
        eng.ps = SimpleNamespace(tp_size=2)
        with pytest.raises(ValueError, match="tensor parallelism"):
            eng.add_request("x", SamplingParams(guide=CHOICE))
    finally:
        eng.ps = ps
    assert not eng.has_work()


def test_service_validates_where_the_request_enters(cpu_engine):
    svc = EngineService(cpu_engine)
    try:
        bad = svc.submit("x", SamplingParams(guide={"regex": "a*?"}))
        with pytest.raises(ValueError, match="lazy"):
            bad.result(timeout=5)
        text, seq = svc.submit("which severity?", SamplingParams(max_tokens=20, temperature=1.0, guide=CHOICE)
                               ).result(timeout=60)
        assert text in CHOICE["choice"] and seq.finish_reason == "stop"
    finally:
        svc.close() if hasattr(svc, "close") else svc.stop()

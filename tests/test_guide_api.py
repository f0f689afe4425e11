"""Constrained decoding at the HTTP surface: the three request forms of /v1/chat/completions, each
400, and /api/v1/analyze with ``parameters.response_schema`` - against a backend that records what
it is asked (no engine)."""
import json

import pytest

from k8s_llm_monitor_amd.llm.service import GenResult, RuleBackend
from k8s_llm_monitor_amd.monitor.app import build_monitor
from k8s_llm_monitor_amd.monitor.cluster.fake import FakeCluster
from k8s_llm_monitor_amd.monitor.config import from_dict

SCHEMA = {"type": "object", "properties": {"severity": {"enum": ["low", "high"]}, "restarts": {"type": "integer"}}}
MSGS = [{"role": "user", "content": "pod default/api restarts: severity?"}]


class Recorder(RuleBackend):
    """Answers like the rule backend and keeps the keyword arguments of every call."""

    provider = "recorder"

    def __init__(self, refuse=None):
        self.calls, self.refuse = [], refuse

    def generate(self, prompt, **kw):
        self.calls.append(kw)
        if self.refuse is not None and kw.get("guide") is not None:
            raise ValueError(self.refuse)
        g = super().generate(prompt)
        return GenResult(**{**g, "text": '{"severity":"low","restarts":3}', "provider": self.provider})


@pytest.fixture()
def mon():
    cfg = from_dict({"k8s": {"watch_namespaces": "default"}, "metrics": {"namespaces": ["default"]},
                     "llm": {"provider": "none", "guide_max_states": 64}})
    assert cfg.llm.guide_max_states == 64 and from_dict({}).llm.guide_max_states == 512
    m = build_monitor(cfg, backend=FakeCluster.build(seed=2), start_manager=False, llm=True)
    m.manager.collect()
    m.analysis.backend = Recorder()
    assert m.app.guide_max_states == 64 and m.analysis.guide_max_states == 64
    return m


def chat(m, **fields):
    r = m.app.handle("POST", "/v1/chat/completions", json.dumps({"messages": MSGS, **fields}).encode())
    return r.code, json.loads(r.body) if r.code == 200 else r.body.decode("utf-8")  # errors are plain text


def test_the_three_request_forms(mon):
    b = mon.analysis.backend
    code, d = chat(mon, response_format={"type": "json_schema", "json_schema": {"name": "f", "schema": SCHEMA}})
    assert code == 200 and b.calls[-1]["guide"] == {"json_schema": SCHEMA}
    assert json.loads(d["choices"][0]["message"]["content"])["severity"] == "low"
    code, _ = chat(mon, guided_choice=["low", "medium", "high"])
    assert code == 200 and b.calls[-1]["guide"] == {"choice": ["low", "medium", "high"]}
    code, _ = chat(mon, guided_regex=r"pod-[a-z]{3}-\d{2}", max_tokens=12)
    assert code == 200 and b.calls[-1]["guide"] == {"regex": r"pod-[a-z]{3}-\d{2}"} and b.calls[-1]["max_tokens"] == 12
    code, _ = chat(mon, response_format={"type": "text"})  # a no-op, like no field at all
    assert code == 200 and "guide" not in b.calls[-1]
    code, _ = chat(mon)
    assert code == 200 and "guide" not in b.calls[-1]


@pytest.mark.parametrize("fields,msg", [
    ({"response_format": {"type": "json_object"}}, "schema is needed"),
    ({"response_format": {"type": "json_schema"}}, "json_schema.schema"),
    ({"response_format": {"type": "json_schema", "json_schema": {"schema": []}}}, "json_schema.schema"),
    ({"response_format": {"type": "grammar"}}, "not supported"),
    ({"response_format": "json"}, "response_format"),
    ({"response_format": {"type": "json_schema", "json_schema": {"schema": {"$ref": "#/defs/x"}}}}, "$ref"),
    ({"response_format": {"type": "json_schema", "json_schema": {"schema": {"type": "string", "pattern": "a"}}}},
     "pattern"),
    ({"guided_regex": "a*?"}, "lazy"),
    ({"guided_regex": "(?=a)a"}, "not supported"),
    ({"guided_regex": 5}, "string"),
    ({"guided_regex": "[ab]{64}"}, "too large"),  # llm.guide_max_states is 64 here
    ({"guided_choice": []}, "non-empty list"),
    ({"guided_choice": ["a", 1]}, "strings"),
    ({"guided_choice": ["a"], "guided_regex": "a"}, "at most one"),
    ({"guided_choice": ["a"], "response_format": {"type": "json_schema", "json_schema": {"schema": SCHEMA}}},
     "at most one"),
])
def test_each_400(mon, fields, msg):
    n = len(mon.analysis.backend.calls)
    code, d = chat(mon, **fields)
    assert code == 400 and msg in d, d
    assert len(mon.analysis.backend.calls) == n  # refused before any generation


def test_a_guide_the_engine_refuses_is_a_400(mon):
    why = "guided decoding is not supported with tensor parallelism (tp_size > 1)"
    mon.analysis.backend = Recorder(refuse=why)
    code, d = chat(mon, guided_choice=["a", "b"])
    assert code == 400 and why in d
    assert chat(mon)[0] == 200


def test_analyze_passes_a_response_schema_through(mon):
    b = mon.analysis.backend
    body = {"type": "root_cause", "parameters": {"response_schema": SCHEMA, "max_tokens": 64}}
    r = mon.app.handle("POST", "/api/v1/analyze", json.dumps(body).encode())
    d = json.loads(r.body)
    assert r.code == 200 and d["status"] == "success" and b.calls[-1]["guide"] == {"json_schema": SCHEMA}
    assert json.loads(d["result"]["answer"]) == {"severity": "low", "restarts": 3}
    r = mon.app.handle("POST", "/api/v1/analyze", b'{"type":"anomaly_detection"}')
    assert r.code == 200 and "guide" not in b.calls[-1]
    for bad in ({"anyOf": []}, "severity", {"type": "string", "maxLength": 100}):
        n = len(b.calls)
        body = {"type": "root_cause", "parameters": {"response_schema": bad}}
        r = mon.app.handle("POST", "/api/v1/analyze", json.dumps(body).encode())
        assert r.code == 400 and len(b.calls) == n
    # the streaming query route is not offered the feature
    body = {"question": "为什么重启?", "guided_choice": ["a"]}
    r = mon.app.handle("POST", "/api/v1/query", json.dumps(body).encode())
    assert r.code == 200 and "guide" not in b.calls[-1]

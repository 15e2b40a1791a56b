"""The host driver of easykv_amd.api — generate and generate_batch — without a GPU: the real driver code over stub caches that only
follow the cache length from each forward's StepPlan.  What is pinned is the control flow that mirrors the reference: modes, geometry,
chunk schedule, the per-token decode rule, EOS handling, ``eos_poll``, ``dense_growth``, the 'random' draws, the printed line.

Against every golden of the real reference: the printed line, the text / perplexity, the number and length of every forward, the
number of evicting forwards and, for recency / random, every evicted range.  The batched driver against the solo driver, sequence by
sequence.  The kernels' own arithmetic is the business of tests/test_hip_generate_*.py."""
import contextlib
import dataclasses
import io
import math
import re
from types import SimpleNamespace

import pytest
import torch

from tests.golden_util import golden_names, load_golden

EVICTING = ("roco", "h2o_head", "tova", "recency", "random")


def _n_evict(plan):
    if not plan.evict or plan.policy not in EVICTING:
        return 0
    return 1 if plan.phase == "decode" else plan.stride


class StubBank:
    def __init__(self, n_layers, hq, h, d, cap, dtype):
        self.n_layers, self.n_q_heads, self.n_kv_heads, self.head_dim, self.cap, self.dtype = n_layers, hq, h, d, cap, dtype
        self.n_slots = [0] * n_layers
        self.kv_quant = None

    def state_init(self, *a, **k):
        pass

    def release_workspace(self, **k):
        pass

    def quantize(self, kind):
        self.kv_quant = kind

    def layout_signature(self):
        return 0


class StubCache:
    """api.BudgetedKVCache as the drivers see it.  ``log``: per forward (n, positions, plan as a dict)."""
    made = 0

    def __init__(self, n_layers, n_q_heads, n_kv_heads, head_dim, cap, device, streaming=False, rope=None, record=False,
                 layer_begin=0, layer_count=None, rope_base=10000.0, dtype=None):
        type(self).made += 1
        self.layer_begin, self.layer_count = layer_begin, n_layers - layer_begin if layer_count is None else layer_count
        self.bank = StubBank(self.layer_count, n_q_heads, n_kv_heads, head_dim, cap, torch.float16 if dtype is None else dtype)
        self.streaming, self.record, self.evictions = streaming, record, []
        self.score_prefix, self.unrotate, self.n_attend, self.plan, self.positions = False, None, 0, None, None
        self.log = []

    def get_seq_length(self, layer_idx=None):
        return self.bank.n_slots[0]

    @contextlib.contextmanager
    def active(self, plan, positions=None):
        self.plan, self.positions, self.n_attend = plan, positions, 0
        yield self

    def attend(self, layer_idx, q, k, v):
        self.n_attend += 1
        if self.n_attend == self.layer_count:
            n = q.shape[2]
            grown = self.bank.n_slots[0] + n - _n_evict(self.plan)
            self.bank.n_slots = [grown] * self.layer_count
            self.log.append((n, self.positions.view(-1).tolist(), dataclasses.asdict(self.plan)))
        return torch.zeros_like(q)


class StubBankBatch:
    def __init__(self, n_seq, n_layers, hq, h, d, cap, device=None, dtype=None):
        self.n_seq, self.n_layers, self.dtype, self.cap = n_seq, n_layers, dtype, cap
        self.lens, self.n_calls = [0] * n_seq, 0

    def adopt(self, i, bank):
        self.lens[i] = bank.n_slots[0]

    def n_slots(self, i):
        return self.lens[i]


class StubCacheBatch:
    """api.BudgetedKVCacheBatch as generate_batch sees it.  ``logs[s]``: per decode forward of sequence s (1, [position], plan)."""
    made = 0
    streaming, unrotate = False, None

    def __init__(self, bat, record=False):
        type(self).made += 1
        self.bat, self.record = bat, record
        self.evictions = [[] for _ in range(bat.n_seq)]
        self.plans, self.live, self.positions, self.n_attend = [], [], None, 0
        self.logs = [[] for _ in range(bat.n_seq)]

    def get_seq_length(self, layer_idx=None):
        return max((self.bat.n_slots(s) for s in self.live), default=0)

    @contextlib.contextmanager
    def active(self, plans, live, positions=None):
        self.plans, self.live, self.positions, self.n_attend = list(plans), list(live), positions, 0
        yield self

    def attend(self, layer_idx, q, k, v):
        assert q.shape[0] == len(self.live) and q.shape[2] == 1
        self.n_attend += 1
        self.bat.n_calls += 1
        if self.n_attend == self.bat.n_layers:
            for row, (s, plan) in enumerate(zip(self.live, self.plans)):
                self.bat.lens[s] += 1 - _n_evict(plan)
                self.logs[s].append((1, [int(self.positions[row, 0])], dataclasses.asdict(plan)))
        return torch.zeros_like(q)


@pytest.fixture
def api(monkeypatch):
    """easykv_amd.api with the three device classes replaced by the stubs, and a sampler that leaves the CPU generator alone: the
    reference's fixtures were produced with the sampler on another generator than the one kv_policy='random' draws from."""
    from easykv_amd import api
    monkeypatch.setattr(api, "BudgetedKVCache", StubCache)
    monkeypatch.setattr(api, "KVBankBatch", StubBankBatch)
    monkeypatch.setattr(api, "BudgetedKVCacheBatch", StubCacheBatch)
    multinomial = torch.multinomial

    def draw(*a, **k):
        state = torch.get_rng_state()
        try:
            return multinomial(*a, **k)
        finally:
            torch.set_rng_state(state)
    monkeypatch.setattr(torch, "multinomial", draw)
    StubCache.made = StubCacheBatch.made = 0
    return api


def _ids(length):
    return torch.arange(length).view(1, -1) % 16


def _solo(api, g, length=None, mode=None, **extra):
    from tests.native_fake_model import NativeFakeModel
    m = g["meta"]
    model = NativeFakeModel(*g["streams"], device="cpu", arch=m["arch"], vocab=m.get("vocab", 16))
    cfg = dict(m["config"], eos_token_ids=m.get("eos_token_ids", [-1]), _record_evictions=True, **extra)
    if m.get("rng_seed") is not None:
        torch.manual_seed(m["rng_seed"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res, cache = api.generate(model, _ids(length or m["length"]), cfg, kv_mode=mode or m["mode"], stride=m["stride"], return_cache=True)
    return res, cache, buf.getvalue().strip()


def _same_result(m, res):
    if m["mode"] == "ppl":
        return abs(res - float(m["result"])) <= 1e-6 * float(m["result"])
    return res == m["result"]


@pytest.mark.parametrize("name", golden_names())
def test_generate_drives_the_reference_forwards(api, name):
    g = load_golden(name)
    m = g["meta"]
    res, cache, line = _solo(api, g)
    assert line == m["printed"]
    assert _same_result(m, res)
    assert [n for n, _, _ in cache.log] == g["out_lens"].tolist()
    evicting = [p for _, _, p in cache.log if p["evict"]]
    assert len(evicting) == len(g["kinds"])
    if m["config"].get("kv_policy", "recency") in ("recency", "random"):
        ranges = [[p["range_start"], p["range_start"] + (1 if p["phase"] == "decode" else p["stride"])] for p in evicting]
        assert ranges == g["ranges"].tolist()


def _eos_cases():
    return [n for n in golden_names() if load_golden(n)["meta"].get("eos_token_ids", [-1]) != [-1]]


@pytest.mark.parametrize("eos_poll", [None, 1, 4, 16])
@pytest.mark.parametrize("name", _eos_cases())
def test_eos_branch_host_side(api, name, eos_poll):
    """The host-side claims of tests/test_hip_generate_parity.py::test_eos_branch_matches_reference."""
    g = load_golden(name)
    m = g["meta"]
    res, cache, line = _solo(api, g, **({} if eos_poll is None else dict(eos_poll=eos_poll)))
    poll = eos_poll or 1
    assert line == m["printed"] and res == m["result"]
    n_tokens = len(m["result"].split())
    assert n_tokens < m["config"]["max_new_tokens"]
    n_evicting = sum(p["evict"] for _, _, p in cache.log)
    assert n_evicting >= len(g["kinds"])
    assert [n for n, _, _ in cache.log][:len(g["out_lens"])] == g["out_lens"].tolist()
    assert cache.host_syncs <= math.ceil(cache.tokens_sampled / poll) + 1
    if poll == 1:
        assert len(cache.log) == m["n_forwards"] and n_evicting == len(g["kinds"])
        assert cache.tokens_sampled == n_tokens and cache.host_syncs == n_tokens
        num = int(re.search(r"[\(\[](\d+)/", m["printed"]).group(1))
        if m["mode"] == "decoding" or (m["mode"] == "auto" and m["printed"].startswith("KV cache budget ratio")):
            expect = num + m["length"]
        elif m["mode"] == "encoding":
            expect = num + n_tokens - 1
        else:
            expect = num
        assert cache.get_seq_length() == expect
    else:
        assert cache.tokens_sampled <= min(m["config"]["max_new_tokens"], (n_tokens + poll - 1) // poll * poll)


def _growth_cases():
    out = []
    for n in golden_names():
        m = load_golden(n)["meta"]
        budget = m["config"].get("budget", 0.5)
        strided = (m["mode"] == "ppl" and budget < 1.0) or (m["mode"] == "auto" and budget <= m["length"])
        if strided and m.get("rng_seed") is None:
            out.append(n)
    return out


@pytest.mark.parametrize("name", _growth_cases())
def test_dense_growth_joins_the_growing_chunks_to_the_prefix(api, name):
    g = load_golden(name)
    m = g["meta"]
    _, base, _ = _solo(api, g)
    res, cache, line = _solo(api, g, dense_growth=True)
    assert line == m["printed"] and _same_result(m, res)
    _, idx, r_idx = api.geometry(m["mode"], m["length"], m["config"]["budget"], m["stride"])
    first = next(f for f, (_, _, p) in enumerate(base.log) if p["evict"])
    assert first == 1 + (idx - r_idx) // m["stride"] and cache.log[0][0] == idx and not cache.log[0][2]["evict"]
    assert cache.log[1:] == base.log[first:]


BATCHES = [("dec_roco", (16, 19, 22, 24)), ("dec_h2o_head", (16, 19, 22, 24)), ("dec_tova", (16, 19, 22, 24)),
           ("dec_roco_gqa", (16, 19, 22, 24)), ("dec_recency", (16, 19, 22, 24)), ("dec_roco_d128", (8, 11, 13, 15, 16)),
           ("auto_to_decoding", (20, 24, 28)), ("auto_roco_s4", (96, 100, 104)),      # GOLDEN_BATCHES of test_hip_generate_batch.py
           ("dec_roco_eos_mid", (16, 19, 22, 24)), ("enc_roco_s4", (100, 104, 108)), ("dec_random", (16, 19, 22, 24))]


@pytest.mark.parametrize("name,lengths", BATCHES, ids=[c[0] for c in BATCHES])
def test_generate_batch_plans_each_sequence_like_its_solo_run(api, name, lengths):
    from tests.batch_fake_model import BatchFakeModel
    g = load_golden(name)
    m = g["meta"]
    assert max(lengths) + m["config"]["max_new_tokens"] <= g["streams"][0].shape[2]      # (every position has a stream row)
    model = BatchFakeModel(*g["streams"], device="cpu", arch=m["arch"], vocab=m.get("vocab", 16))
    cfg = dict(m["config"], eos_token_ids=m.get("eos_token_ids", [-1]), _record_evictions=True)
    if m.get("rng_seed") is not None:
        torch.manual_seed(m["rng_seed"])
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res, cache = api.generate_batch(model, [_ids(n) for n in lengths], cfg, kv_mode=m["mode"], stride=m["stride"], return_cache=True)
    lines = buf.getvalue().strip().split("\n")
    assert len(res) == len(lines) == len(lengths)
    assert lengths[0] == m["length"] and res[0] == m["result"] and lines[0] == m["printed"]
    for i, n in enumerate(lengths):
        sres, scache, sline = _solo(api, g, length=n)
        steps = [f for f in scache.log if f[2]["phase"] == "decode"]
        assert res[i] == sres and lines[i] == sline, (i, n)
        if m["config"]["kv_policy"] == "random":      # (the draws interleave across sequences: the counts only)
            assert len(cache.logs[i]) == len(steps) and sum(f[2]["evict"] for f in cache.logs[i]) == sum(f[2]["evict"] for f in steps)
        else:
            assert cache.logs[i] == steps, (i, n)
    assert cache.bat.n_calls == model.n_batched_forwards * model.config.num_hidden_layers
    assert model.n_batched_forwards == max(len(l) for l in cache.logs)


def test_refusals_come_before_any_cache(api):
    from oracle.fake_model import make_streams
    from tests.batch_fake_model import BatchFakeModel
    model = BatchFakeModel(*make_streams(2, 4, 4, 32, 64, seed=1), device="cpu")
    ids, gen = [_ids(16), _ids(20)], dict(kv_policy="roco", budget=8, max_new_tokens=4)
    for extra, mode, match in ((dict(streaming=True), "decoding", "streaming"), (dict(kv_quant="fp8"), "decoding", "kv_quant"),
                               (dict(hipgraph=True), "decoding", "hipgraph"), ({}, "ppl", "ppl")):
        with pytest.raises(ValueError, match=match):
            api.generate_batch(model, ids, dict(gen, **extra), kv_mode=mode)
    for bad in ([], [torch.zeros(2, 8, dtype=torch.long)]):
        with pytest.raises(ValueError, match="prompts"):
            api.generate_batch(model, bad, gen, kv_mode="decoding")
    for extra, mode, match in ((dict(kv_quant="int8"), "decoding", "must be None or 'fp8'"), (dict(kv_quant="fp8", streaming=True), "decoding", "no RoPE-on-read build"),
                               (dict(kv_quant="fp8"), "ppl", "no decode phase to quantise"), (dict(kv_quant="fp8"), "decoding", "needs head_dim 64 or 128"),
                               (dict(kv_dtype="float32"), "decoding", "must be 'float16', 'bfloat16' or 'auto'"),
                               (dict(kv_dtype="bfloat16", streaming=True), "decoding", "RoPE-on-read has no bf16 build")):
        with pytest.raises(ValueError, match=match):
            api.generate(model, ids[0], dict(gen, **extra), kv_mode=mode)
    model.layer_shard = SimpleNamespace(world=2, rank=0, begin=0, count=1)
    with pytest.raises(ValueError, match="layer-sharded"):
        api.generate_batch(model, ids, gen, kv_mode="decoding")
    with pytest.raises(ValueError, match="not supported on a layer-sharded model"):
        api.generate(model, ids[0], dict(gen, kv_quant="fp8"), kv_mode="decoding")
    assert StubCache.made == StubCacheBatch.made == 0

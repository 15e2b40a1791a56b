"""Which phase order the one-launch decode step is planned with (ekv_step_info field `fused_order`, a dry run: no GPU): the mixed
mode only where order K exists and pays — head_dim 128, one query head per KV head, a scored policy, slot-indexed rows, 4-wave
workgroups and more than 512 heads in the launch — and EKV_FUSED_ORDER = 0 / 1 / 2 forces all F / mixed / all K (read once per
process, so every setting is asked in a child process)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_MODE = 1

CHILD = r"""
import ctypes, json
from tests.test_dispatch_table import _case, _structs
from easykv_amd import _lib
lib = _lib.load()
slot = dict(phases=16, phys_extent=2112, n_split=1)
cases = dict(
    bench=dict(n_layers=32, **slot), layers18=dict(n_layers=18, **slot), h2o=dict(n_layers=32, policy=1, win_tail=100, **slot),
    tova=dict(n_layers=32, policy=3, **slot),
    ordered_rows=dict(n_layers=32, phys_extent=2112, n_split=1), eight_waves=dict(n_layers=16, **slot), few_heads=dict(n_layers=4, **slot),
    gqa=dict(n_layers=32, hq=32, h=16, **slot), d64=dict(n_layers=32, head_dim=64, **slot),
    long_rows=dict(n_layers=32, phases=16, n_split=1, n_slots=3000, cap=3008, phys_extent=3008, roco_k1=2100))
out = {}
for name, kw in cases.items():
    bank, st = _structs(_case(**kw))
    info = (ctypes.c_int32 * 10)()
    assert lib.ekv_step_info(ctypes.byref(bank), ctypes.byref(st), info, 10) == 0
    out[name] = [info[1], info[9]]
print(json.dumps(out))
"""


def _ask(mode):
    env = {k: v for k, v in os.environ.items() if not k.startswith("EKV_FUSED_ORDER")}
    if mode is not None:
        env["EKV_FUSED_ORDER"] = str(mode)
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.splitlines()[-1])


@pytest.mark.parametrize("mode", [None, 0, 1, 2])
def test_planned_phase_order(mode):
    from easykv_amd import _build
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    got = _ask(mode)
    m = DEFAULT_MODE if mode is None else mode
    for name, (fused, order) in got.items():
        assert fused == 1, name                                  # every case is a one-launch decode step
    for name in ("bench", "layers18", "h2o", "tova"):            # > 512 heads of the flagship instance on slot-indexed rows
        assert got[name][1] == m, (name, got[name])
    # 4 layers (128 heads): under two workgroups per CU the mixed mode has nothing to mix; all K still applies
    assert got["few_heads"][1] == (2 if m == 2 else 0), got["few_heads"]
    for name in ("ordered_rows", "eight_waves", "gqa", "d64", "long_rows"):      # instances without order K
        assert got[name][1] == 0, (name, got[name])

"""The bf16 entry points of the C ABI on a CPU (nothing is dereferenced, nothing is launched): the `_typed` calls are exported and
declared; EKV_DTYPE_F16 answers exactly as the untyped calls; a bf16 step of plain keys is planned exactly as the fp16 step (rc, the 9
ekv_step_info fields, workspace bytes) over the whole grid of tests/test_dispatch_table.py; RoPE-on-read has no bf16 build
(EKV_E_UNSUPPORTED, no launches); any other dtype is EKV_E_ARG.  The A/B switches are read once per process, so the grid runs in a
child process with them cleared."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16 = 0, 1


def _lib():
    from easykv_amd import _build, _lib as L
    if not os.path.exists(_build.LIB):
        _build.build_lib()
    return L, L.load()


def test_typed_symbols_are_exported_and_declared():
    L, lib = _lib()
    header = open(os.path.join(ROOT, "include", "easykv_hip.h")).read()
    declared = set(re.findall(r"\b(ekv_[a-z_]+)\s*\(", header))
    for name in ("ekv_workspace_bytes_typed", "ekv_step_check_typed", "ekv_step_info_typed", "ekv_step_attend_typed"):
        assert name in declared and name in L.EXPORTS and hasattr(lib, name), name
    assert "EKV_DTYPE_F16 = 0, EKV_DTYPE_BF16 = 1" in header
    assert (L.DTYPE_F16, L.DTYPE_BF16) == (F16, BF16)


def answers(lib, bank, st, dtype):
    """check rc, info rc, the 9 info fields, workspace bytes of one (bank, step) in `dtype` (None = the untyped calls)."""
    b, s = ctypes.byref(bank), ctypes.byref(st)
    info = (ctypes.c_int32 * 9)(*([-7] * 9))
    if dtype is None:
        return [lib.ekv_step_check(b, s), lib.ekv_step_info(b, s, info, 9)] + list(info) + [lib.ekv_workspace_bytes(b, s)]
    return ([lib.ekv_step_check_typed(b, s, dtype), lib.ekv_step_info_typed(b, s, dtype, info, 9)] + list(info) +
            [lib.ekv_workspace_bytes_typed(b, s, dtype)])


def typed_table():
    """[case][variant][field]: variants = untyped, F16, BF16, dtype 2, dtype -1."""
    from tests.test_dispatch_table import _structs, cases
    _, lib = _lib()
    rows = []
    for c in cases():
        bank, st = _structs(c)
        rows.append([answers(lib, bank, st, d) for d in (None, F16, BF16, 2, -1)])
    return np.array(rows, dtype=np.int64)


def test_bf16_plans_as_fp16_over_the_dispatch_grid(tmp_path):
    from tests.test_dispatch_table import SWITCHES, cases
    _lib()
    path = str(tmp_path / "typed.npy")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    r = subprocess.run([sys.executable, "-m", "tests.test_bf16_dispatch_cpu", "--emit", path], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    t = np.load(path)
    cs = cases()
    rope = np.array([c["rope_on_read"] for c in cs], dtype=bool)
    untyped, f16, bf16, d2, dm1 = (t[:, i] for i in range(5))
    # EKV_DTYPE_F16 is the untyped call
    bad = np.nonzero((f16 != untyped).any(axis=1))[0]
    assert len(bad) == 0, [(int(i), cs[i], untyped[i].tolist(), f16[i].tolist()) for i in bad[:3]]
    # plain keys: bf16 answers exactly as fp16
    bad = np.nonzero((bf16[~rope] != f16[~rope]).any(axis=1))[0]
    assert len(bad) == 0, [(bf16[~rope][i].tolist(), f16[~rope][i].tolist()) for i in bad[:3]]
    # RoPE-on-read: every step fp16 accepts is refused in bf16 with no launches; the ones fp16 refuses keep their code
    acc = rope & (f16[:, 0] == 0)
    assert acc.sum() > 20
    assert (bf16[acc, 0] == -2).all() and (bf16[acc, 1] == 0).all() and (bf16[acc, 2 + 8] == 0).all() and (bf16[acc, 2 + 1] == 0).all()
    assert (bf16[acc, -1] == f16[acc, -1]).all()      # (the tiling and the workspace layout are still the fp16 plan's)
    ref = rope & (f16[:, 0] != 0)
    assert (bf16[ref, 0] == f16[ref, 0]).all()
    # any other dtype value: EKV_E_ARG from check and info
    for bad_dt in (d2, dm1):
        assert (bad_dt[:, 0] == -1).all() and (bad_dt[:, 1] == -1).all()
    # the grid covers every plain-key path of a bf16 step: fused decode, split decode, chunk kernels (wide and 16x16), one-launch chunk
    assert (bf16[~rope, 2 + 1] == 1).any() and (bf16[~rope, 2 + 3] == 1).any() and (bf16[~rope, 2 + 2] == 1).any()


if __name__ == "__main__":
    if sys.argv[1] == "--emit":
        np.save(sys.argv[2], typed_table())

"""The kernel instances of the library (easykv_amd/csrc/ekv_instances.def) on a CPU: no instance is lost.

The manifest is the only list of instances; easykv_amd/_build.py derives one object per line from it.  The object names are unique,
equal — as a set — the names the library had when every instance was a .hip file of its own (tests/golden/dispatch/instances.txt: the
base names of csrc/*.hip at that commit; a new instance adds its line there), and after a build every one of them exists and is not
older than the manifest."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _names():
    from easykv_amd import _build
    return [name for name, _ in _build.objects()]


def test_object_names_are_unique():
    names = _names()
    assert len(names) == len(set(names)), sorted(n for n in set(names) if names.count(n) > 1)


def test_object_names_are_the_recorded_ones():
    with open(os.path.join(ROOT, "tests", "golden", "dispatch", "instances.txt")) as f:
        recorded = f.read().split()
    assert len(recorded) == len(set(recorded))
    names = set(_names())
    assert names == set(recorded), (sorted(names - set(recorded)), sorted(set(recorded) - names))


def test_every_manifest_line_is_parsed():
    """A line the build's pattern does not see would silently drop an instance: every FAMILY( at the start of a line is one."""
    from easykv_amd import _build
    with open(_build.MANIFEST) as f:
        lines = [ln for ln in f if ln.startswith("EKV_")]
    inst = _build.instances()
    assert len(inst) == len(lines) and all(fam in _build.FAMILIES for fam, _ in inst)
    assert [ln.split("(")[0] for ln in lines] == [fam for fam, _ in inst]


def test_every_object_is_built_and_not_older_than_the_manifest():
    from easykv_amd import _build
    _build.build_lib()
    t = os.path.getmtime(_build.MANIFEST)
    for name in _names():
        obj = os.path.join(_build.OBJ, name + ".o")
        assert os.path.exists(obj), name
        assert os.path.getmtime(obj) >= t, name

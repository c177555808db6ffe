"""tests/golden/reference_loader.py, the module every fixture generator loads the reference through: the registration of
packages, files and stubs on a small package written for the test, the one rule for where the reference lies, and that
importing a generator has no side effects.  Needs neither the reference nor a GPU."""
import os
import subprocess
import sys
import textwrap
import types

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import reference_loader as rl  # noqa: E402


@pytest.fixture
def clean_modules():
    before = set(sys.modules)
    yield
    for name in set(sys.modules) - before:
        del sys.modules[name]


def write_tree(root):
    """<root>/pcdet/{ext/stub.py, pkg/sub/{sibling, child}.py}: child imports its sibling and, two levels up, the stubbed leaf.
    No __init__.py anywhere, and ext/stub.py raises, so the test passes only if the loader's packages and stub are used."""
    files = {"pcdet/ext/stub.py": "raise ImportError('the real extension must not be imported')\n",
             "pcdet/pkg/sub/sibling.py": "VALUE = 7\n",
             "pcdet/pkg/sub/child.py": "from . import sibling\nfrom ...ext.stub import stub_fn\nSEEN = (sibling.VALUE, stub_fn())\n"}
    for rel, text in files.items():
        path = os.path.join(str(root), *rel.split("/"))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    return str(root)


@pytest.mark.parametrize("real_paths", [False, True])
def test_load_registers_parents_stubs_and_files_in_order(tmp_path, clean_modules, real_paths):
    root = write_tree(tmp_path)
    stub_fn = lambda: "stub"                                              # noqa: E731
    mods = rl.load(root, "ldr_t", ["pkg.sub.sibling", "pkg.sub.child"], stubs={"ext.stub": {"stub_fn": stub_fn}},
                   real_paths=real_paths)
    assert [m.__name__ for m in mods] == ["ldr_t.pkg.sub.sibling", "ldr_t.pkg.sub.child"]
    sibling, child = mods
    assert child.SEEN == (7, "stub") and child.sibling is sibling and child.stub_fn is stub_fn
    for name in ("ldr_t", "ldr_t.pkg", "ldr_t.pkg.sub", "ldr_t.ext", "ldr_t.ext.stub"):        # the missing parents
        assert isinstance(sys.modules[name], types.ModuleType) and hasattr(sys.modules[name], "__path__"), name
    assert sys.modules["ldr_t"].pkg.sub.child is child and sys.modules["ldr_t"].ext.stub.stub_fn is stub_fn
    assert sys.modules["ldr_t"].__path__ == [os.path.join(root, "pcdet")]
    assert sys.modules["ldr_t.pkg.sub"].__path__ == ([os.path.join(root, "pcdet", "pkg", "sub")] if real_paths else [])
    # a second call keeps what is registered: the parents are the same objects, a stub given as a module is taken as it is
    pkg = sys.modules["ldr_t.pkg"]
    given = types.ModuleType("given")
    again, = rl.load(root, "ldr_t", ["pkg.sub.sibling"], stubs={"ext.other": given}, real_paths=real_paths)
    assert sys.modules["ldr_t.pkg"] is pkg and again is not sibling and pkg.sub.sibling is again
    assert sys.modules["ldr_t.ext.other"] is given and sys.modules["ldr_t.ext"].other is given


def test_package_and_module(tmp_path, clean_modules):
    root = write_tree(tmp_path)
    top = rl.package("ldr_p", os.path.join(root, "pcdet", "pkg"))
    sub = rl.package("ldr_p.sub", None, marker=3)
    assert sys.modules["ldr_p"] is top and top.sub is sub and sub.marker == 3 and sub.__path__ == []
    path = os.path.join(root, "pcdet", "pkg", "sub", "sibling.py")
    m = rl.module("ldr_p.sub.sibling", path)
    assert sys.modules["ldr_p.sub.sibling"] is m and sub.sibling is m and m.VALUE == 7
    # sys.modules is filled before the file runs: a file may look itself up
    me = os.path.join(root, "me.py")
    with open(me, "w") as f:
        f.write("import sys\nFOUND = sys.modules[__name__].__name__\n")
    assert rl.module("ldr_me", me).FOUND == "ldr_me"


@pytest.mark.parametrize("argv, env, want", [
    (["make_x.py", "/from/argv"], {"PDA_REFERENCE": "/a", "PDA_REFERENCE_ROOT": "/b"}, "/from/argv"),
    (["make_x.py"], {"PDA_REFERENCE": "/a", "PDA_REFERENCE_ROOT": "/b"}, "/a"),
    (["make_x.py"], {"PDA_REFERENCE": "/a"}, "/a"),
    (["make_x.py"], {"PDA_REFERENCE_ROOT": "/b"}, "/b"),
    (["make_x.py"], {}, None),
])
def test_reference_root(monkeypatch, argv, env, want):
    monkeypatch.setattr(sys, "argv", argv)
    for name in ("PDA_REFERENCE", "PDA_REFERENCE_ROOT"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    if want is not None:
        assert rl.reference_root() == want
        return
    with pytest.raises(SystemExit) as e:
        rl.reference_root()
    assert isinstance(e.value.code, str) and e.value.code.strip()          # a message, not a bare status


def test_importing_a_generator_has_no_side_effects():
    """One child process imports every tests/golden/make_*.py by file name, with no argument and neither variable set."""
    script = textwrap.dedent("""
        import glob, importlib.util, os, sys
        import numpy as np
        import torch
        golden = sys.argv.pop()
        sys.path.insert(0, golden)
        assert sys.argv == ["-c"]
        cuda, float_tensor, float_, perm = torch.Tensor.cuda, torch.cuda.FloatTensor, torch.Tensor.float, np.random.permutation
        paths = sorted(glob.glob(os.path.join(golden, "make_*.py")))
        assert len(paths) >= 25
        for path in paths:
            name = os.path.splitext(os.path.basename(path))[0]
            spec = importlib.util.spec_from_file_location(name, path)
            spec.loader.exec_module(importlib.util.module_from_spec(spec))
            bad = [k for k in sys.modules if k.startswith(("pcdet", "once_eval", "numba", "SharedArray", "torch_scatter"))]
            assert not bad, (name, bad)
            assert torch.Tensor.cuda is cuda and torch.cuda.FloatTensor is float_tensor and torch.Tensor.float is float_, name
            assert np.random.permutation is perm and np.random.permutation.__self__ is np.random.mtrand._rand, name
        print("imported", len(paths))
    """)
    env = {k: v for k, v in os.environ.items() if k not in ("PDA_REFERENCE", "PDA_REFERENCE_ROOT")}
    r = subprocess.run([sys.executable, "-c", script, GOLDEN], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "imported" in r.stdout

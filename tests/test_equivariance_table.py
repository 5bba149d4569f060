"""The table of tests/equivariance_cases.py covers the package: every public name of kerneldensityestimate.jl_amd/__init__.py --
what it imports and the functions it defines -- is in exactly one row's `entries` (run under rescaling and translation by
tests/test_gpu_equivariance.py) or in `EXCLUDED` (with the reason).  So is every public function and class of a module of
the package that __init__.py imports nothing from -- a family whose surface is methods plus a module, as `refit` and
`transport` are --, under its qualified name (`transport.sinkhorn`); which modules those are is found, not listed.  A new
entry fails here until it has a law or a stated reason.  Needs no GPU and no library: the modules are parsed as text, the
table is imported without running a row."""
import glob
import os
import re

from tests import equivariance_cases as cases

PACKAGE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kerneldensityestimate.jl_amd")
INIT = os.path.join(PACKAGE, "__init__.py")


def _code(text):
    """a module text without its docstrings and comments"""
    text = re.sub(r'"""[\s\S]*?"""', " ", text)
    return re.sub(r"#[^\n]*", " ", text)


def exported(text, imports=True, module=None):
    """the public names of a module text: what its `from ... import` statements bind (the `as` name where there is one; left
    out with imports=False) and the functions and classes it defines at top level; names with a leading underscore are
    private.  Docstrings and comments are ignored.  `module`: the names are qualified by it, `module.name`."""
    text = _code(text)
    names = []
    if imports:
        for m in re.finditer(r"^from\s+[.\w]+\s+import\s+(\([^)]*\)|[^\n]*)", text, flags=re.M):
            for part in m.group(1).strip("()").split(","):
                words = part.split()
                if not words:
                    continue
                names.append(words[2] if len(words) == 3 and words[1] == "as" else words[0])
    names += re.findall(r"^(?:def|class)\s+([A-Za-z_]\w*)", text, flags=re.M)
    prefix = "" if module is None else module + "."
    return sorted(prefix + n for n in names if not n.startswith("_"))


def imported_modules(text):
    """the modules of the package a module text imports from: X of `from .X import ...` and of `from . import X, Y as Z`"""
    text = _code(text)
    found = set(re.findall(r"^from\s+\.(\w+)\s+import\b", text, flags=re.M))
    for m in re.finditer(r"^from\s+\.\s+import\s+(\([^)]*\)|[^\n]*)", text, flags=re.M):
        found |= {part.split()[0] for part in m.group(1).strip("()").split(",") if part.split()}
    return found


def unexported_modules(init_text, package=PACKAGE):
    """{module: its text} over the package's *.py whose name has no leading underscore and from which __init__.py imports
    nothing: their public functions and classes are reached as `package.module.name` (and as methods) alone"""
    used = imported_modules(init_text)
    out = {}
    for path in sorted(glob.glob(os.path.join(package, "*.py"))):
        name = os.path.splitext(os.path.basename(path))[0]
        if name.startswith("_") or name in used:
            continue
        with open(path) as f:
            out[name] = f.read()
    return out


def test_the_parser_reads_imports_and_definitions_and_ignores_comments():
    text = '''"""docstring: from .nothing import ghost"""
from ._lib import Err, PATH, lib as _private  # noqa: F401  (from .c import commented)
from .a import (one, two,  # noqa
                three as four)
from .b import five as six
# from .c import seven


def eight() -> int:
    return 8


def _nine():
    pass


class Ten:
    def method(self):
        pass
'''
    assert exported(text) == sorted(["Err", "PATH", "one", "two", "four", "six", "eight", "Ten"])
    assert imported_modules(text) == {"_lib", "a", "b"}
    # a second module text, one that __init__ imports nothing from: its definitions alone, qualified by the module
    other = '''"""def ghost(): a docstring"""
from __future__ import annotations

import numpy as np

from . import _lib, manifold as _mf
from ._lib import addr, f64p
from .loglik import _dims

KEEP = 0


def _helper(x):
    return x


def first(p, q=None):  # def commented(): no
    def inner():
        pass
    return inner


class Second:
    def method(self):
        pass
'''
    assert exported(other, imports=False, module="family") == ["family.Second", "family.first"]
    assert "annotations" in exported(other) and "addr" in exported(other)   # (what imports=False leaves out)
    assert imported_modules(other) == {"_lib", "manifold", "loglik"}


def test_the_modules_that_init_does_not_re_export_are_discovered(tmp_path):
    with open(INIT) as f:
        init = f.read()
    found = unexported_modules(init)
    assert {"refit", "transport"} <= set(found), sorted(found)
    assert not any(m.startswith("_") for m in found) and "density" not in found and "product" not in found
    # a package made up here: `b` and `_c` are imported from or private, `d` is the family that ships as methods plus a module
    for name, text in (("__init__", "from .b import one\nfrom . import e as _e\n"), ("b", "def one():\n    pass\n"),
                       ("_c", "def two():\n    pass\n"), ("d", "def three():\n    pass\n\n\ndef _four():\n    pass\n"),
                       ("e", "def five():\n    pass\n")):
        (tmp_path / (name + ".py")).write_text(text)
    made = unexported_modules((tmp_path / "__init__.py").read_text(), str(tmp_path))
    assert sorted(made) == ["d"] and exported(made["d"], imports=False, module="d") == ["d.three"]


def test_every_public_name_has_a_law_or_a_reason():
    with open(INIT) as f:
        init = f.read()
    want = exported(init)
    assert len(want) >= 100 and "evaluate_hess" in want and "device_count" in want  # (the parser found the imports)
    modules = unexported_modules(init)
    assert {"refit", "transport"} <= set(modules), sorted(modules)   # (the discovery found the families that ship as methods)
    for name, text in modules.items():
        want = want + exported(text, imports=False, module=name)
    assert "transport.sinkhorn" in want and "refit.refit_device" in want
    where = {}
    for name, place in cases.all_entries():
        where.setdefault(name, []).append(place)
    missing = [n for n in want if n not in where]
    assert not missing, f"no row and no reason for: {missing}"
    twice = {n: p for n, p in where.items() if len(p) > 1}
    assert not twice, f"in more than one place: {twice}"
    unknown = sorted(n for n in where if n not in want)
    assert not unknown, (f"not a public name of kerneldensityestimate.jl_amd/__init__.py, nor of a module it imports nothing "
                         f"from: {unknown}")


def test_the_table_is_consistent():
    names = [r.name for r in cases.ROWS]
    assert len(names) == len(set(names))
    for name, reason in cases.EXCLUDED.items():
        assert isinstance(reason, str) and len(reason.split()) >= 4, name
    for r in cases.ROWS:
        assert r.entries and callable(r.call) and r.laws, r.name
        # the family's model, by its file in tests/, or in so many words that there is none
        named = re.findall(r"tests/(\w+\.py)", r.model)
        assert "no model" in r.model or named, r.name
        for f in named:
            assert os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), f)), (r.name, f)
        for out, law in r.laws.items():
            assert law.kind in ("bits", "add", "inv", "rel", "near", "search"), (r.name, out)
            assert law.t in ("same", "pos", "leaves", "close", None), (r.name, out)
            if law.kind != "bits":  # not exact: the operation responsible is on record
                assert law.why and len(law.why.split()) >= 4, (r.name, out)
        assert set(cases.scales_of(r)) <= set(cases.K)
        if r.scales is not None:  # a restricted row says why, citing the reference
            assert r.restriction and "1e-6" in r.restriction, r.name
    assert sorted(cases.K) == [-80, -30, 30, 80]
    assert cases.BASE_CASES == [(4, 129, 257), (5, 257, 129), (7, 129, 257), (8, 130, 3)]
    # the largest exponent of any bit law stays inside fp64 with base values in [2^-150, 2^150]
    assert (max(D for D, _, _ in cases.BASE_CASES) + 2) * max(cases.K) + 150 < 1023

"""The table of tests/equivariance_cases.py covers the package: every public name of kerneldensityestimate.jl_amd/__init__.py --
what it imports and the functions it defines -- is in exactly one row's `entries` (run under rescaling and translation by
tests/test_gpu_equivariance.py) or in `EXCLUDED` (with the reason).  A new entry fails here until it has a law or a stated
reason.  Needs no GPU and no library: __init__.py is parsed as text, the table is imported without running a row."""
import os
import re

from tests import equivariance_cases as cases

INIT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "kerneldensityestimate.jl_amd", "__init__.py")


def exported(text):
    """the public names of a module text: what its `from ... import` statements bind (the `as` name where there is one) and the
    functions and classes it defines at top level; names with a leading underscore are private.  Docstrings and comments are
    ignored."""
    text = re.sub(r'"""[\s\S]*?"""', " ", text)
    text = re.sub(r"#[^\n]*", " ", text)
    names = []
    for m in re.finditer(r"^from\s+[.\w]+\s+import\s+(\([^)]*\)|[^\n]*)", text, flags=re.M):
        for part in m.group(1).strip("()").split(","):
            words = part.split()
            if not words:
                continue
            names.append(words[2] if len(words) == 3 and words[1] == "as" else words[0])
    names += re.findall(r"^(?:def|class)\s+([A-Za-z_]\w*)", text, flags=re.M)
    return sorted(n for n in names if not n.startswith("_"))


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


def test_every_public_name_has_a_law_or_a_reason():
    with open(INIT) as f:
        want = exported(f.read())
    assert len(want) >= 100 and "evaluate_hess" in want and "device_count" in want  # (the parser found the imports)
    where = {}
    for name, place in cases.all_entries():
        where.setdefault(name, []).append(place)
    missing = [n for n in want if n not in where]
    assert not missing, f"no row and no reason for: {missing}"
    twice = {n: p for n, p in where.items() if len(p) > 1}
    assert not twice, f"in more than one place: {twice}"
    unknown = sorted(n for n in where if n not in want)
    assert not unknown, f"not a public name of kerneldensityestimate.jl_amd/__init__.py: {unknown}"


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

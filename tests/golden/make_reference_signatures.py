"""Generates tests/golden/reference_signatures.json: the method signatures of the reference's `kde!`, `evaluateDualTree`,
`gibbs1` and `prodAppxMSGibbsS`, in the canonical form test_julia_shim_syntax.py compares the shim's overrides against
(positional `name::Type` list without defaults, keyword names in order, the `where` variables the positional arguments
use).  Parsed with the test's own functions from the reference package's source directory:
    python tests/golden/make_reference_signatures.py <KernelDensityEstimate.jl checkout>/src
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.test_julia_shim_syntax import _canonical, _function_signatures, strip_code  # noqa: E402

SOURCES = (("kde!", "KDE01.jl"), ("evaluateDualTree", "DualTree01.jl"), ("gibbs1", "MSGibbs01.jl"),
           ("prodAppxMSGibbsS", "MSGibbs01.jl"))


def main(src):
    out = {}
    for name, f in SOURCES:
        code = strip_code(open(os.path.join(src, f)).read())
        methods = [_canonical(s, w) for s, w in _function_signatures(code, name)]
        assert methods, name
        out[name] = {"file": "src/" + f,
                     "methods": [{"positional": list(p), "keywords": list(k), "where": w} for p, k, w in methods]}
    path = os.path.join(ROOT, "tests", "golden", "reference_signatures.json")
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])

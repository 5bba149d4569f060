"""Scalar-register spills of the headline sampler instantiation, read from the built library's code-object metadata.

gibbs_lean_kernel<double, 6, 4, 8> (BASELINE config 3) parks the scalar registers it cannot keep in lanes of vector
registers; every reload is a vector instruction in front of the scalar address arithmetic of a step
(profiles/scalar_spills.md, scripts/spill_map.py).  The compiler's own count is in the code object's notes, next to the
vector-register count tests/test_lean_registers.py reads: no GPU is needed.

    .sgpr_spill_count   before: 384 (one build for every staging mode)
                        now:    141 (the build for plans that are resident throughout; its staged twin: 246)

The count is held at the value reached: a change that raises it has to say why."""
import os
import re
import subprocess

import pytest

from tests.test_lean_registers import KERNEL, LIB, TARGET, _bundles, _fatbin, _tool

PARENT_SGPR_SPILLS = 384
MAX_SGPR_SPILLS = 141


def test_config3_sampler_scalar_spills(tmp_path):
    bundler, readelf = _tool("clang-offload-bundler"), _tool("llvm-readelf")
    if not bundler or not readelf:
        pytest.skip("clang-offload-bundler / llvm-readelf not found")
    assert os.path.exists(LIB), f"{LIB} is missing: build the library first"
    with open(LIB, "rb") as f:
        fat = _fatbin(f.read())
    src, obj = str(tmp_path / "bundle.hipfb"), str(tmp_path / "code.co")
    for bundle in _bundles(fat):
        with open(src, "wb") as f:
            f.write(bundle)
        subprocess.run([bundler, "--type=o", f"--targets={TARGET}", f"--input={src}", f"--output={obj}", "--unbundle"],
                       check=True, capture_output=True)
        with open(obj, "rb") as f:
            if KERNEL.encode() not in f.read():
                continue
        notes = subprocess.run([readelf, "--notes", obj], check=True, capture_output=True, text=True).stdout
        entries = re.split(r"\n\s+- \.", notes)
        mine = [e for e in entries if re.search(r"\.name:\s+" + re.escape(KERNEL) + r"\s", e)]
        assert len(mine) == 1, len(mine)
        spills = int(re.search(r"\.sgpr_spill_count:\s+(\d+)", mine[0]).group(1))
        print(f"gibbs_lean_kernel<double,6,4,8,false,false>: {spills} scalar registers spilled (before: {PARENT_SGPR_SPILLS})")
        assert MAX_SGPR_SPILLS < PARENT_SGPR_SPILLS
        assert spills <= MAX_SGPR_SPILLS, spills
        return
    raise AssertionError(f"{KERNEL} is in no code object of {LIB}")

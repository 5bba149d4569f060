"""Register budget of the headline sampler instantiation, read from the built library's code-object metadata.

gibbs_lean_kernel<double, 6, 4, 8> (BASELINE config 3) shares the device with the next call's table build only while it
allocates at most 216 vector registers (profiles/r06_experiments.md section 10); beyond that the call loses 12 us at an
unchanged kernel time.  The compiler's own figures are in the code object's notes: no GPU is needed to read them."""
import os
import re
import shutil
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(os.path.dirname(HERE), "kerneldensityestimate.jl_amd", "libkdehip.so")
KERNEL = "_ZN6kdehip17gibbs_lean_kernelIdLi6ELi4ELi8ELb0ELb0EEEvNS_7PlanDevENS_7RunArgsE"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
MAX_VGPRS = 216


def _tool(name):
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin"), "/opt/rocm/lib/llvm/bin"):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    return shutil.which(name)


def _fatbin(blob):
    """The bytes of the ELF64 section .hip_fatbin."""
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", blob, 0x3A)
    sec = [struct.unpack_from("<IIQQQQ", blob, shoff + i * shentsize) for i in range(shnum)]
    names = sec[shstrndx]
    for name, _, _, _, off, size in sec:
        end = blob.index(b"\0", names[4] + name)
        if blob[names[4] + name:end] == b".hip_fatbin":
            return blob[off:off + size]
    raise AssertionError("no .hip_fatbin section")


def _bundles(fat):
    """The offload bundles of the section, one per translation unit (compressed: 'CCOB' + its total size; plain: the
    bundle's table of entries), with zero padding between them."""
    pos, plain = 0, b"__CLANG_OFFLOAD_BUNDLE__"
    while pos < len(fat):
        if fat[pos] == 0:
            pos += 1
        elif fat.startswith(b"CCOB", pos):
            version, = struct.unpack_from("<H", fat, pos + 4)
            total, = struct.unpack_from("<Q" if version >= 3 else "<I", fat, pos + 8)
            yield fat[pos:pos + total]
            pos += total
        elif fat.startswith(plain, pos):
            n, = struct.unpack_from("<Q", fat, pos + len(plain))
            p, end = pos + len(plain) + 8, 0
            for _ in range(n):
                off, size, idlen = struct.unpack_from("<QQQ", fat, p)
                end = max(end, off + size)
                p += 24 + idlen
            end = max(end, p - pos)
            yield fat[pos:pos + end]
            pos += end
        else:
            raise AssertionError(f"unknown bundle at offset {pos} of .hip_fatbin")


def test_config3_sampler_register_budget(tmp_path):
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
        # the kernel's entry of amdhsa.kernels: from its .name back to the previous entry's, forward to the next one's
        entries = re.split(r"\n\s+- \.", notes)
        mine = [e for e in entries if re.search(r"\.name:\s+" + re.escape(KERNEL) + r"\s", e)]
        assert len(mine) == 1, len(mine)
        vgprs = int(re.search(r"\.vgpr_count:\s+(\d+)", mine[0]).group(1))
        spills = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", mine[0]).group(1))
        print(f"gibbs_lean_kernel<double,6,4,8,false,false>: {vgprs} VGPRs, {spills} spilled")
        assert vgprs <= MAX_VGPRS and spills == 0, (vgprs, spills)
        return
    raise AssertionError(f"{KERNEL} is in no code object of {LIB}")

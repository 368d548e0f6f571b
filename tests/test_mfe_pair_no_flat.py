"""mfe_pair_kernel reaches device memory with global_* instructions only (no GPU needed).

The kernel's loop reads its arguments again in every pass, so the compiler cannot
trace a pointer among them to the argument segment: dereferenced as it stands, it
is a generic pointer and the access a flat_* instruction, which counts on lgkmcnt
as well as vmcnt -- every `s_waitcnt lgkmcnt(0)` that ends an LDS read batch then
also waits for the loads from L2 / HBM in flight.  The accesses therefore go
through fold_common.hpp's gld() / gst().  A plain dereference added later brings
a flat instruction back without any other sign: this test compiles mfe_pair.hip
to assembly (device code only, about 12 s) and looks.
"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "addapt_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("mfe_pair_asm") / "mfe_pair.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    "--cuda-device-only", "-S", os.path.join(CSRC, "mfe_pair.hip"), "-o", out], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    with open(out) as f:
        return f.read()


def _kernels(asm):
    """The instruction lines of every mfe_pair_kernel instantiation, by symbol."""
    out, name = {}, None
    for line in asm.split("\n"):
        m = re.match(r"^(_Z\w*mfe_pair_kernel\w*):", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif re.match(r"^\s*\.end_amdhsa_kernel|^\.Lfunc_end", line):
            name = None
        elif name and re.match(r"^\s+[a-z]\w+(\s|$)", line):
            out[name].append(line.strip())
    return out


def test_no_flat_instruction(asm):
    ks = _kernels(asm)
    assert len(ks) == 2, list(ks)   # NM = 64 and NM = 100
    for name, lines in ks.items():
        assert len(lines) > 10000, (name, len(lines))
        flat = [l for l in lines if l.startswith("flat_")]
        assert not flat, (name, len(flat), flat[:8])
        # and the accesses are there as global ones: the restore, the tables, the write-back
        for op in ("global_load_dwordx2", "global_load_ushort", "global_store_dwordx4", "global_atomic_add"):
            assert any(l.startswith(op) for l in lines), (name, op)

#!/usr/bin/env python3
"""Variant builds of the engine into addapt_amd/_lib/ablate/lib_<name>.so, on
top of addapt_amd/_build.build_gpu (its source list and compile flags).
Select one with ADX_LIB=addapt_amd/_lib/ablate/lib_<name>.so (tools/gpu_run.sh).

  name=<git rev or "tree">:<files, comma-separated>:<flags>
      those sources (and generated *.inc) at that revision, the rest from the
      working tree; the flags ("__" for spaces) go to every source:
        tools/build_variant.py base=tree:: stamp=tree::-DADX_STAMP old=HEAD:mfe_cells.hip:
  --mfe-roles  name/ROLES4/FLAGS   mfe_cells.hip on blocks the generator seeds with
      other role costs (tools/gen_mfe_blocks.py ADX_GEN_ROLES4, "wave:cost,...")
  --pair-roles name/ROLES4/FLAGS   the same for mfe_pair.hip (ADX_GEN_PAIR_ROLES4)
"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from addapt_amd import _build  # noqa: E402

OUT = os.path.join(_build.OUT, "ablate")


def build(name, flags, tmp, files=(), rev="tree", gen_env=None):
    d = os.path.join(tmp, name)
    os.makedirs(d)
    for f in files:   # a replaced source sits beside the *.inc it includes
        if rev == "tree":
            shutil.copy(os.path.join(_build.CSRC, f), d)
        else:
            with open(os.path.join(d, f), "wb") as out:
                out.write(subprocess.check_output(["git", "-C", ROOT, "show", "%s:addapt_amd/csrc/%s" % (rev, f)]))
    if gen_env:
        subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_mfe_blocks.py")],
                              env=dict(os.environ, ADX_GEN_OUT=d, **gen_env), stdout=subprocess.DEVNULL)
    replace = {f: os.path.join(d, f) for f in files if f in _build.GPU_SOURCES}
    return _build.build_gpu(force=True, out_dir=os.path.join(OUT, name), lib_name="../lib_%s.so" % name,
                            extra_flags=flags.replace("__", " ").split(), replace=replace)


def main(argv):
    mode = None
    with tempfile.TemporaryDirectory() as tmp:
        for a in argv:
            if a in ("--mfe-roles", "--pair-roles"):
                mode = a
            elif mode:
                name, roles, flags = (a.split("/") + ["", ""])[:3]
                src, env = (("mfe_cells.hip", {"ADX_GEN_ONLY": "cells", "ADX_GEN_ROLES4": roles}) if mode == "--mfe-roles"
                            else ("mfe_pair.hip", {"ADX_GEN_ONLY": "pair", "ADX_GEN_PAIR_ROLES4": roles}))
                print(build(name, flags, tmp, files=[src], gen_env=env))
            else:
                name, rest = a.split("=", 1)
                rev, files, flags = (rest.split(":", 2) + ["", ""])[:3]
                print(build(name, flags, tmp, files=[f for f in files.split(",") if f], rev=rev or "tree"))


if __name__ == "__main__":
    main(sys.argv[1:])

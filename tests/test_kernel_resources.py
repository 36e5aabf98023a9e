"""The resource notes of the built library's gfx950 kernels, read the way tools/kernel_diff.py reads them: no kernel uses scratch
memory but the one that is known to (bu_uastc_multi_kernel<0,512,2,true,false> spills one VGPR, 8 bytes per lane,
measured as a net win).  A refactor or a compiler that makes another kernel spill shows up here, on the CPU, before any GPU run."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPILLS = {"bu_uastc_multi_kernelILi0ELi512ELi2ELb1ELb0EE": 8}  # mangled template-id -> bytes of private segment


def _kernel_diff():
    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_only_the_known_kernel_uses_scratch():
    kd = _kernel_diff()
    if not kd.tools_present():
        pytest.skip("the LLVM tools that unbundle and read a gfx950 code object are not installed")
    from basisu_rs_amd import build

    ks = kd.kernels(build.LIB if os.path.exists(build.LIB) else build.build_hip())
    assert len(ks) > 100, "the code object holds %d kernels" % len(ks)
    scratch = {name: k["scratch"] for name, k in ks.items() if k["scratch"]}
    want = {name: b for name in ks for tid, b in SPILLS.items() if tid in name}
    assert len(want) == len(SPILLS), "the kernel known to spill is not in the library"
    assert scratch == want

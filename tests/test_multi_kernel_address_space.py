"""The multi-run kernels rebuild a run's addresses from integers (the run record travels through LDS), so nothing tells the compiler which address space they
point into unless the code does: a block load through such a pointer is a flat_load, which counts on lgkmcnt as well as vmcnt and forbids counted waits.
Read the way tools/kernel_diff.py reads the built library: no bu_uastc_multi_kernel instantiation holds a flat load or store."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kernel_diff():
    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_no_multi_run_kernel_uses_flat_memory_instructions():
    kd = _kernel_diff()
    if not kd.tools_present():
        pytest.skip("the LLVM tools that unbundle and read a gfx950 code object are not installed")
    from basisu_rs_amd import build

    ks = kd.kernels(build.LIB if os.path.exists(build.LIB) else build.build_hip())
    multi = {name: k for name, k in ks.items() if "bu_uastc_multi_kernel" in name}
    assert len(multi) >= 4, "the code object holds %d multi-run kernels" % len(multi)
    flat = {name: [ln for ln in k["code"] if ln.startswith(("flat_load", "flat_store"))] for name, k in multi.items()}
    assert not {name: lns[:4] for name, lns in flat.items() if lns}
    # (the tile accesses are there, and global: every instantiation loads its blocks and stores its results)
    for name, k in multi.items():
        assert any(ln.startswith("global_load_dwordx4") for ln in k["code"]), name
        assert any(ln.startswith("global_store_dword") for ln in k["code"]), name


# The whole-tile BC7 / ASTC multi-run kernels issue a tile's result stores last (bu_kernels.hpp, STORES_LAST), and what that buys rests on the compiler placing NO
# vmcnt wait between those stores and the next tile's prefetch loads: vmcnt counts loads and stores in issue order, so any such wait is a wait for the stores'
# acknowledgement.  The placement depends on the wait-count pass's bookkeeping (values consumed on every path, one full wait in front of the loop); a compiler that
# brings the wait back costs 2 % of the headline and changes no result, so it is asserted here.  In these kernels the loop's tail, the next tile's phase A and the
# prefetch of phase B follow each other in the listing (the strip-layout kernels are laid out differently and are not read this way).
STORES_LAST_WHOLE = ("bu_uastc_multi_kernelILi1ELi256ELi4ELb1ELb1EE", "bu_uastc_multi_kernelILi0ELi256ELi4ELb1ELb1EE")


def _waits_behind_the_result_stores(code):
    """listing order from the loop's last `sc1` result store, across a barrier, to the next tile's first prefetch load: the vmcnt waits met on the way"""
    def is_store(ln):
        return ln.startswith("global_store_dwordx4") and "sc1" in ln

    for i in reversed([i for i, ln in enumerate(code) if is_store(ln)]):
        barrier, waits = False, []
        for ln in code[i + 1:]:
            if ln.startswith("s_endpgm") or is_store(ln):
                break
            barrier = barrier or ln.startswith("s_barrier")
            if ln.startswith("s_waitcnt") and "vmcnt" in ln:
                waits.append(ln)
            if ln.startswith(("global_load_dwordx4", "flat_load_dwordx4")):
                if barrier:
                    return waits
                break
    return None


def test_no_wait_on_the_result_stores_before_the_next_prefetch():
    kd = _kernel_diff()
    if not kd.tools_present():
        pytest.skip("the LLVM tools that unbundle and read a gfx950 code object are not installed")
    from basisu_rs_amd import build

    ks = kd.kernels(build.LIB if os.path.exists(build.LIB) else build.build_hip())
    for tid in STORES_LAST_WHOLE:
        (name,) = [n for n in ks if tid in n]
        waits = _waits_behind_the_result_stores(ks[name]["code"])
        assert waits is not None, "%s: no stretch from the result stores to the prefetch loads in the listing -- read its loop by hand" % tid
        assert waits == [], "%s waits for vmcnt behind its result stores: %r" % (tid, waits)

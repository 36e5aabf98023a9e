"""bu_etc1s_rect_job and bu_etc1s_transcode_rects_device in the three places that spell them: include/basisu_hip.h, the ctypes binding and the (uncompiled)
Rust binding -- field by field and parameter by parameter, as tests/test_rect_capi.py does for the UASTC call -- and the eight kernels in the built library."""
import ctypes
import os
import re

from basisu_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("d_idx", "const uint32_t*", "*const u32", ctypes.c_void_p), ("d_alpha_idx", "const uint32_t*", "*const u32", ctypes.c_void_p),
          ("in_blocks_per_row", "uint32_t", "u32", ctypes.c_uint32), ("x0", "uint32_t", "u32", ctypes.c_uint32), ("y0", "uint32_t", "u32", ctypes.c_uint32),
          ("w", "uint32_t", "u32", ctypes.c_uint32), ("h", "uint32_t", "u32", ctypes.c_uint32), ("d_out", "void*", "*mut c_void", ctypes.c_void_p),
          ("out_pitch_bytes", "uint64_t", "u64", ctypes.c_uint64), ("index_base", "uint64_t", "u64", ctypes.c_uint64)]
PARAMS = [("bu_context*", "*mut bu_context", ctypes.c_void_p), ("bu_target", "c_int", ctypes.c_int), ("size_t", "usize", ctypes.c_size_t),
          ("const bu_etc1s_rect_job*", "*const bu_etc1s_rect_job", ctypes.POINTER(_lib.Etc1sRectJob)), ("const uint32_t*", "*const u32", ctypes.c_void_p),
          ("uint32_t", "u32", ctypes.c_uint32), ("const void*", "*const c_void", ctypes.c_void_p), ("uint32_t", "u32", ctypes.c_uint32),
          ("uint64_t*", "*mut u64", ctypes.c_void_p), ("void*", "*mut c_void", ctypes.c_void_p)]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "basisu_hip.h")).read(), flags=re.S)


def test_struct_fields_agree():
    hdr = _header()
    body = re.search(r"typedef struct bu_etc1s_rect_job \{(.*?)\}\s*bu_etc1s_rect_job;", hdr, flags=re.S).group(1)
    c_fields = []
    for line in body.split(";"):
        line = " ".join(line.split())
        if not line:
            continue
        typ, names = re.match(r"^(.*?[\s\*])(\w+(?:\s*,\s*\w+)*)$", line).groups()
        c_fields += [(n.strip(), typ.strip().replace(" *", "*")) for n in names.split(",")]
    assert c_fields == [(n, c) for n, c, _, _ in FIELDS]
    rs = re.sub(r"//.*", "", open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read())
    rm = re.search(r"#\[repr\(C\)\][^{]*pub struct bu_etc1s_rect_job\s*\{(.*?)\}", rs, flags=re.S).group(1)
    r_fields = [(f.split(":")[0].replace("pub", "").strip(), f.split(":")[1].strip()) for f in rm.split(",") if ":" in f]
    assert r_fields == [(n, r) for n, _, r, _ in FIELDS]
    assert [(n, t) for n, t in _lib.Etc1sRectJob._fields_] == [(n, t) for n, _, _, t in FIELDS]
    assert ctypes.sizeof(_lib.Etc1sRectJob) == 64 and _lib.Etc1sRectJob.d_out.offset == 40
    assert _lib.Etc1sRectJob.in_blocks_per_row.offset == 16 and _lib.Etc1sRectJob.out_pitch_bytes.offset == 48 and _lib.Etc1sRectJob.index_base.offset == 56


def test_function_declarations_agree():
    hdr = _header()
    m = re.search(r"bu_status\s+bu_etc1s_transcode_rects_device\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    c_params = [re.match(r"^(.*?)(\w+)$", " ".join(a.split())).group(1).strip().replace(" *", "*") for a in m.group(1).split(",")]
    assert c_params == [c for c, _, _ in PARAMS]
    rs = re.sub(r"//.*", "", open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read())
    m = re.search(r"pub\(crate\) fn bu_etc1s_transcode_rects_device\s*\((.*?)\)\s*->\s*([^;]+);", rs, flags=re.S)
    assert [a.split(":", 1)[1].strip() for a in " ".join(m.group(1).split()).split(",")] == [r for _, r, _ in PARAMS]
    assert m.group(2).strip() == "c_int"
    assert "bu_etc1s_transcode_rects_device" in _lib.SYMBOLS
    fn = _lib.load().bu_etc1s_transcode_rects_device
    assert list(fn.argtypes) == [t for _, _, t in PARAMS] and fn.restype is ctypes.c_int
    # the declaration is crate-visible; the crate's users get it through a public wrapper of lib.rs that takes the jobs as a slice
    lib_rs = re.sub(r"//.*", "", open(os.path.join(ROOT, "rust", "src", "lib.rs")).read())
    w = re.search(r"pub unsafe fn etc1s_transcode_rects_device\s*\((.*?)\)\s*->\s*Result<\(\)>\s*\{(.*?)\n\}", lib_rs, flags=re.S)
    assert [a.split(":", 1)[1].strip() for a in " ".join(w.group(1).split()).split(",")] == [
        "*mut ffi::bu_context", "c_int", "&[ffi::bu_etc1s_rect_job]", "*const u32", "u32", "*const core::ffi::c_void", "u32", "*mut u64", "*mut core::ffi::c_void"]
    assert ("ffi::bu_etc1s_transcode_rects_device(ctx, target, jobs.len(), jobs.as_ptr(), d_endpoints, n_endpoints, d_selectors, n_selectors, d_status, stream)"
            in w.group(2))
    # and the Python driver has the method
    from basisu_rs_amd import Context

    assert callable(Context.etc1s_transcode_rects_device)


def test_eight_rectangle_kernels_are_built_without_scratch_and_flat_accesses():
    """the kernels rebuild every address from the integers of the job table, so the index loads must say "global" themselves (as the UASTC rectangle kernels' block
    loads do: tests/test_rect_capi.py); read the way tools/kernel_diff.py reads the built library"""
    import importlib.util

    import pytest

    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    if not kd.tools_present():
        pytest.skip("the LLVM tools that unbundle and read a gfx950 code object are not installed")
    from basisu_rs_amd import build

    ks = {n: k for n, k in kd.kernels(build.LIB if os.path.exists(build.LIB) else build.build_hip()).items() if "bu_etc1s_rects_kernel" in n}
    assert sorted(int(re.search(r"rects_kernelILi(\d+)E", n).group(1)) for n in ks) == [2, 4, 6, 7, 8, 9, 11, 12]
    for name, k in ks.items():
        assert k["scratch"] == 0, name
        assert not [ln for ln in k["code"] if ln.startswith(("flat_load", "flat_store"))][:4], name
        assert any(ln.startswith("global_load_dword ") for ln in k["code"]) and any(ln.startswith("global_store_dword") for ln in k["code"]), name

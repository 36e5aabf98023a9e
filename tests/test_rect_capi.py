"""bu_rect_job and bu_uastc_transcode_rects_device in the three places that spell them: include/basisu_hip.h, the ctypes binding and the (uncompiled)
Rust binding.  tests/test_capi_symbols.py checks names and, for the parameter types it knows, every extern fn of rust/src/ffi.rs; a pointer to this struct is
not among those types, so the declaration and the struct are checked here, field by field and parameter by parameter."""
import ctypes
import os
import re

from basisu_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [("d_in", "const void*", "*const c_void", ctypes.c_void_p), ("in_blocks_per_row", "uint32_t", "u32", ctypes.c_uint32), ("x0", "uint32_t", "u32", ctypes.c_uint32),
          ("y0", "uint32_t", "u32", ctypes.c_uint32), ("w", "uint32_t", "u32", ctypes.c_uint32), ("h", "uint32_t", "u32", ctypes.c_uint32),
          ("d_out", "void*", "*mut c_void", ctypes.c_void_p), ("out_pitch_bytes", "uint64_t", "u64", ctypes.c_uint64), ("index_base", "uint64_t", "u64", ctypes.c_uint64)]
PARAMS = [("bu_context*", "*mut bu_context"), ("bu_target", "c_int"), ("size_t", "usize"), ("const bu_rect_job*", "*const bu_rect_job"), ("uint64_t*", "*mut u64"),
          ("void*", "*mut c_void")]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "basisu_hip.h")).read(), flags=re.S)


def test_struct_fields_agree():
    hdr = _header()
    body = re.search(r"typedef struct bu_rect_job \{(.*?)\}\s*bu_rect_job;", hdr, flags=re.S).group(1)
    c_fields = []
    for line in body.split(";"):
        line = " ".join(line.split())
        if not line:
            continue
        typ, names = re.match(r"^(.*?[\s\*])(\w+(?:\s*,\s*\w+)*)$", line).groups()
        c_fields += [(n.strip(), typ.strip().replace(" *", "*")) for n in names.split(",")]
    assert c_fields == [(n, c) for n, c, _, _ in FIELDS]
    rs = re.sub(r"//.*", "", open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read())
    rm = re.search(r"#\[repr\(C\)\][^{]*pub struct bu_rect_job\s*\{(.*?)\}", rs, flags=re.S).group(1)
    r_fields = [(f.split(":")[0].replace("pub", "").strip(), f.split(":")[1].strip()) for f in rm.split(",") if ":" in f]
    assert r_fields == [(n, r) for n, _, r, _ in FIELDS]
    assert [(n, t) for n, t in _lib.RectJob._fields_] == [(n, t) for n, _, _, t in FIELDS]
    assert ctypes.sizeof(_lib.RectJob) == 56 and _lib.RectJob.d_out.offset == 32 and _lib.RectJob.index_base.offset == 48


def test_function_declarations_agree():
    hdr = _header()
    m = re.search(r"bu_status\s+bu_uastc_transcode_rects_device\s*\(([^;]*?)\)\s*;", hdr, flags=re.S)
    c_params = [re.match(r"^(.*?)(\w+)$", " ".join(a.split())).group(1).strip().replace(" *", "*") for a in m.group(1).split(",")]
    assert c_params == [c for c, _ in PARAMS]
    rs = re.sub(r"//.*", "", open(os.path.join(ROOT, "rust", "src", "ffi.rs")).read())
    m = re.search(r"fn bu_uastc_transcode_rects_device\s*\((.*?)\)\s*->\s*([^;]+);", rs, flags=re.S)
    assert [a.split(":", 1)[1].strip() for a in " ".join(m.group(1).split()).split(",")] == [r for _, r in PARAMS]
    assert m.group(2).strip() == "c_int"
    assert "bu_uastc_transcode_rects_device" in _lib.SYMBOLS
    # the declaration is crate-visible; the crate's users get it through a public wrapper of lib.rs that takes the jobs as a slice
    lib_rs = re.sub(r"//.*", "", open(os.path.join(ROOT, "rust", "src", "lib.rs")).read())
    w = re.search(r"pub unsafe fn transcode_rects_device\s*\((.*?)\)\s*->\s*Result<\(\)>\s*\{(.*?)\n\}", lib_rs, flags=re.S)
    assert [a.split(":", 1)[1].strip() for a in " ".join(w.group(1).split()).split(",")] == ["*mut ffi::bu_context", "c_int", "&[ffi::bu_rect_job]", "*mut u64",
                                                                                               "*mut core::ffi::c_void"]
    assert "ffi::bu_uastc_transcode_rects_device(ctx, target, jobs.len(), jobs.as_ptr(), d_status, stream)" in w.group(2)


def test_one_rectangle_kernel_per_target_is_built_without_flat_accesses():
    """the kernels rebuild every address from the integers of the job table, so the block loads must say "global" themselves (as the multi-run kernels' do:
    tests/test_multi_kernel_address_space.py); read the way tools/kernel_diff.py reads the built library"""
    import importlib.util

    import pytest

    spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
    kd = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kd)
    if not kd.tools_present():
        pytest.skip("the LLVM tools that unbundle and read a gfx950 code object are not installed")
    from basisu_rs_amd import build

    ks = {n: k for n, k in kd.kernels(build.LIB if os.path.exists(build.LIB) else build.build_hip()).items() if "bu_uastc_rects_kernel" in n}
    assert sorted(int(re.search(r"rects_kernelILi(\d+)E", n).group(1)) for n in ks) == [0, 1, 2, 3, 4, 6, 7, 8, 9, 11, 12]
    for name, k in ks.items():
        assert k["scratch"] == 0, name
        assert not [ln for ln in k["code"] if ln.startswith(("flat_load", "flat_store"))][:4], name
        assert any(ln.startswith("global_load_dwordx4") for ln in k["code"]) and any(ln.startswith("global_store_dword") for ln in k["code"]), name

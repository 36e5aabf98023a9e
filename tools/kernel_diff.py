#!/usr/bin/env python3
"""tools/kernel_diff.py OLD.so NEW.so : do two builds of the library hold the same gfx950 kernels?

Unbundles the gfx950 code object from each library's .hip_fatbin and compares, kernel by kernel (mangled name), the resource
notes (VGPRs, SGPRs, static LDS, scratch) and the disassembly with addresses and PC-relative literals stripped.  Prints one line
per kernel that differs or exists on one side only, then a summary; exit status 0 when the name sets, notes and code are all equal.
-v prints a line for every kernel; --diff prints a unified diff of each differing kernel's code.

kernels(lib) is also what tests/test_kernel_resources.py reads the built library with."""
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM_DIRS = ("/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin")
TOOLS = ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf", "llvm-objdump")
NOTES = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"), ("scratch", ".private_segment_fixed_size"))


def tool(name):
    """path of an LLVM tool of the ROCm installation (or of PATH), None if absent"""
    for d in LLVM_DIRS:
        p = os.path.join(d, name)
        if os.access(p, os.X_OK):
            return p
    return shutil.which(name)


def tools_present():
    return all(tool(t) for t in TOOLS)


def _run(name, *args):
    return subprocess.run([tool(name)] + list(args), check=True, capture_output=True, text=True).stdout


def _normalise(lines):
    """instruction text without the address comment; the literals of an s_getpc_b64 / s_add_u32 / s_addc_u32 address pair replaced"""
    out, pcrel = [], ()
    for ln in lines:
        ln = ln.split("//")[0].strip()
        if not ln:
            continue
        m = re.match(r"s_getpc_b64 s\[(\d+):(\d+)\]", ln)
        if m:
            pcrel = ("s_add_u32 s%s, s%s, " % (m.group(1), m.group(1)), "s_addc_u32 s%s, s%s, " % (m.group(2), m.group(2)))
        else:
            for p in pcrel:
                if ln.startswith(p):
                    ln = p + "PCREL"
        out.append(ln)
    return out


def kernels(lib):
    """mangled kernel name -> {"vgpr", "sgpr", "lds", "scratch": int, "code": [normalised instruction lines]} of the gfx950 code object"""
    with tempfile.TemporaryDirectory() as tmp:
        fat, dev = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.o")
        _run("llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat)
        _run("clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--input=" + fat, "--output=" + dev)
        notes = _run("llvm-readelf", "--notes", dev)
        asm = _run("llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", dev)
    out = {}
    for entry in re.split(r"^  - \.agpr_count:", notes, flags=re.M)[1:]:
        field = dict(re.findall(r"^    (\.\w+):\s+(\S+)$", entry, flags=re.M))
        out[field[".name"]] = {k: int(field[f]) for k, f in NOTES}
    code = {}
    name = None
    for ln in asm.splitlines():
        m = re.match(r"^<(.+)>:$", ln)
        if m:
            name = m.group(1)
            code[name] = []
        elif name is not None:
            code[name].append(ln)
    for name, k in out.items():
        k["code"] = _normalise(code[name])
    return out


def main(argv):
    flags = [a for a in argv if a.startswith("-")]
    paths = [a for a in argv if not a.startswith("-")]
    if len(paths) != 2 or not tools_present():
        sys.stderr.write(__doc__ if len(paths) != 2 else "the LLVM tools (%s) are not installed\n" % ", ".join(TOOLS))
        return 2
    old, new = kernels(paths[0]), kernels(paths[1])
    same = differ = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print("%s ONLY  %s" % ("old" if name in old else "new", name))
            continue
        o, n = old[name], new[name]
        res = " ".join("%s %d" % (k, n[k]) if o[k] == n[k] else "%s %d->%d" % (k, o[k], n[k]) for k, _ in NOTES)
        notes_eq, code_eq = all(o[k] == n[k] for k, _ in NOTES), o["code"] == n["code"]
        same += notes_eq and code_eq
        differ += not (notes_eq and code_eq)
        if "-v" in flags or not (notes_eq and code_eq):
            print("%s  notes %s  code %s  %s  (%s)" % ("same  " if notes_eq and code_eq else "DIFFER", "equal" if notes_eq else "differ",
                                                     "equal" if code_eq else "differs (%d -> %d instructions)" % (len(o["code"]), len(n["code"])),
                                                     name, res))
        if "--diff" in flags and not code_eq:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(o["code"], n["code"], "old", "new", lineterm="", n=2))
    names_eq = set(old) == set(new)
    print("%d kernels old, %d new, names %s; %d identical, %d differ" % (len(old), len(new), "equal" if names_eq else "DIFFER", same, differ))
    return 0 if names_eq and differ == 0 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

#!/usr/bin/env python3
"""Compare the gfx950 instruction streams of two csrc trees, kernel by kernel, for the files given on the command line.

    python tools/isa_compare.py <parent csrc> <new csrc> file.hip [file.hip ...]

Any file of csrc can be given (headers are picked up from each tree); without files, the bf16 GEMM family the tool was
first written for.  Each file is compiled in both trees with build.py's flags plus `--cuda-device-only -S`.  Per kernel
the instruction lines are compared as text after dropping comments and the function number in `.LBB<n>_` labels.
Kernels are matched by demangled name; the template arguments that selected a retired GEMM variant are dropped from the
parent's names (RETIRED), so a parent kernel that matches nothing on the new side is one of the retired instantiations;
RETIRED also holds plain renames.  A kernel that is not in the parent's file of the same name is looked up in the other
files named, so a kernel that moved between two files is paired when both are given.
For kernels that differ, the compiler's resource-usage remarks of both sides are printed.  Read the instruction counts
too: a helper that can fall off its end without a return compiles silently into kernels of one instruction.  No GPU
needed.
"""
import difflib, importlib.util, os, re, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# compared when no file is named on the command line; any file of csrc can be named there
FILES = ["gemm_bf16.hip", "gemm_nt.hip", "gemm_ln.hip", "gemm_small.hip", "wgrad.hip"]
RETIRED = [(r"(gemm_bf16_kernel<\d+, \w+), 0, true>", r"\1>"), (r"(wgrad_kernel<\w+), true>", r"\1>"),
           (r"wgrad_group_kernel<true>", "wgrad_group_kernel"), (r"(gemm_nt_mul_kernel<\d+), true, true>", r"\1>"),
           (r"^(cwlt::)?particle_release_kernel$", r"\1particle_release_kernel<false>"),
           (r"^(cwlt::)?particle_release_bank_kernel$", r"\1particle_release_kernel<true>")]


def build_py():
    pkg = next(d for d in sorted(os.listdir(ROOT)) if os.path.exists(os.path.join(ROOT, d, "build.py")))
    spec = importlib.util.spec_from_file_location("cwlt_build", os.path.join(ROOT, pkg, "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def kernels(csrc, name, b, retired):
    """{demangled kernel name: (instruction lines, resource remarks)} of one file, and its compile time."""
    t0 = time.time()
    r = subprocess.run([b.HIPCC] + b.FLAGS + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                              os.path.join(csrc, name), "-o", "-"], capture_output=True, text=True)
    dt = time.time() - t0
    if r.returncode:
        sys.exit(r.stderr)
    res = {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]:
        res[blk.split()[0]] = re.findall(r"remark:\s+(\w[^\n]*?) \[-Rpass", blk)
    out = {}
    for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^(?:\t\.section|\.Lfunc_end\d+:)", r.stdout, re.S | re.M):
        if ".amdhsa_kernel " + m.group(1) not in r.stdout:
            continue
        nm = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        nm = re.sub(r"^void |\(.*$", "", nm)
        for pat, rep in (RETIRED if retired else []):
            nm = re.sub(pat, rep, nm)
        body = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*$", "", l)).strip() for l in m.group(2).splitlines()]
        out[nm] = ([l for l in body if l], res.get(m.group(1), []))
    return out, dt


def main():
    old_dir, new_dir, files = sys.argv[1], sys.argv[2], sys.argv[3:] or FILES
    b = build_py()
    olds, news = {f: kernels(old_dir, f, b, True) for f in files}, {f: kernels(new_dir, f, b, False) for f in files}
    for f in files:
        (own, t_old), (new, t_new) = olds[f], news[f]
        print("%s: %d -> %d kernels, compile %.1f s -> %.1f s" % (f, len(own), len(new), t_old, t_new))
        for nm in sorted(new):
            old = next((o for o in [own] + [olds[x][0] for x in files if x != f] if nm in o), None)
            if old is None:
                print("  new only   %s" % nm)
                continue
            d = [l for l in difflib.unified_diff(old[nm][0], new[nm][0], lineterm="", n=0) if l[:2] not in ("--", "++", "@@")]
            print("  %-10s %s (%d instructions)" % ("identical" if not d else "%d lines" % len(d), nm, len(new[nm][0])))
            if d:
                print("\n".join("      " + l for l in d))
                print("      parent: " + "; ".join(old[nm][1]) + "\n      new:    " + "; ".join(new[nm][1]))
        gone = sorted(set(own) - set().union(*(news[x][0] for x in files)))
        if gone:
            print("  parent only (%d): %s" % (len(gone), ", ".join(gone)))


if __name__ == "__main__":
    main()

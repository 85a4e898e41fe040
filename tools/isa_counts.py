#!/usr/bin/env python3
"""Development helper: static instruction counts of one kernel in a gfx950 assembly listing, by kind, for the whole kernel and for
its wave-level LU region.
   hipcc -O3 --offload-arch=gfx950 -std=c++17 --cuda-device-only -S -o sampler_a.s coulombgas_amd/csrc/cg_k_sampler_a.hip
   python tools/isa_counts.py sampler_a.s [mangled-name-prefix]
The LU region of the single-wave sampler is taken from its first column broadcast (the first quad_perm DPP move of the kernel) to the
start of the closing logarithm behind the last column step (the conversion of the product's exponent to double: the first
v_cvt_f64_i32 after the last quad_perm DPP move)."""
import re, sys

KERNEL = "_Z6k_mcmcILi2ELi16ELi16ELi64ELi13EE"


def body(path, prefix):
    out, on = [], False
    for ln in open(path):
        if not on:
            on = ln.startswith(prefix) and ln.rstrip().split(":")[0].startswith(prefix) and ":" in ln
            continue
        if ln.startswith(".Lfunc_end"):
            break
        s = ln.split(";")[0].strip()
        if s and not s.endswith(":") and not s.startswith("."):
            out.append(s)
    return out


def kinds(ins):
    c = dict(total=len(ins), VALU=0, SALU=0, LDS=0, MFMA=0, flat_load=0, global_load=0, global_store=0, v_writelane=0, v_readlane=0,
             v_mov_b32=0, s_nop=0, s_waitcnt=0, v_cndmask=0, exec_writes=0)
    for s in ins:
        op = s.split()[0]
        if op.startswith("v_mfma"): c["MFMA"] += 1
        elif op.startswith("v_"): c["VALU"] += 1
        elif op.startswith("s_"): c["SALU"] += 1
        elif op.startswith("ds_"): c["LDS"] += 1
        for k in ("flat_load", "global_load", "global_store", "v_writelane", "v_readlane", "s_nop", "s_waitcnt", "v_cndmask"):
            if op.startswith(k): c[k] += 1
        if op.startswith("v_mov_b32"): c["v_mov_b32"] += 1
        if re.match(r"s_\w+ exec\b", s) or re.match(r"s_\w+_saveexec", s): c["exec_writes"] += 1
    return c


def lu_region(ins):
    q = [i for i, s in enumerate(ins) if "quad_perm" in s]
    if not q:
        return []
    end = next((i for i in range(q[-1], len(ins)) if ins[i].startswith("v_cvt_f64_i32")), len(ins))
    return ins[q[0]:end]


if __name__ == "__main__":
    prefix = sys.argv[2] if len(sys.argv) > 2 else KERNEL
    ins = body(sys.argv[1], prefix)
    k, l = kinds(ins), kinds(lu_region(ins))
    print("%-14s %8s %8s" % (prefix[:14], "kernel", "LU region"))
    for name in k:
        print("%-14s %8d %8d" % (name, k[name], l[name]))

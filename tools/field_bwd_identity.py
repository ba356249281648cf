#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device-assembly listings of csrc/field_fused.hip.

The check behind a refactor of the field kernels that must not change the machine code. Needs
no GPU. Compile the parent's and the new source with the Makefile's flags for field_fused.o
plus `--cuda-device-only -S`:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -fno-honor-nans -mno-amdgpu-ieee \
          -mllvm -amdgpu-mfma-vgpr-form=1 -mllvm -amdgpu-sched-strategy=max-ilp \
          --cuda-device-only -S field_fused.hip -o side.s

    tools/field_bwd_identity.py parent.s new.s -o profiles/field_bwd_refactor.json

Per kernel the text from its label to its end, .amdhsa_ block included, is compared as one
string, after every mangled kernel name has been replaced by a neutral key (the backward
kernel's positional template arguments of the parent and its named form of today give the same
key) and the function numbers of local labels have been dropped. The register, scratch and LDS
figures are the .amdhsa_ numbers. Exit status 0: same kernels, all identical.
"""
import argparse
import json
import re
import subprocess
import sys

# parent spelling bwd_rt_kernel<W, NHD, FAST, ROWS, BF, REF, HG, S>: (FAST, ROWS, REF, HG) -> form
COLOR = {"true": "FastColor", "false": "GeneralColor"}
GRADS = {"true": "F16Grads", "false": "F32Grads"}


def old_form(fast, rows, ref, hg):
    if ref == "0":
        return "Build<%s, %s>" % (COLOR[fast], "GatheredRows" if rows == "true" else "DenseRows")
    if ref == "1":
        return "RefF32Rows<%s>" % COLOR[fast]
    if ref == "2":
        return "RefF16Rows<%s, %s>" % (COLOR[fast], GRADS[hg])
    return "%s<%s>" % ({"4": "PosPass", "3": "ListPass"}[ref], GRADS[hg])


def kernel_key(demangled):
    m = re.search(r"bwd_rt_kernel<(.*)>\(anr::field::Args", demangled)
    if not m:
        return demangled
    args = m.group(1).replace("anr::field::", "")
    parts = [p.strip() for p in re.split(r",\s*(?![^<]*>)", args)]
    if len(parts) == 8:  # the parent's positional flags
        w, nhd, fast, rows, bf, ref, hg, s = parts
        form = old_form(fast, rows, ref, hg)
    else:
        w, nhd, bf, s, form = parts
    return "bwd_rt_kernel W=%s NHD=%s %s S=%s %s" % (w, nhd, "bf16" if bf == "true" else "f16", s, form)


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names) + "\n", capture_output=True,
                         text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


AMDHSA = {
    "accum_offset": ".amdhsa_accum_offset",
    "next_free_vgpr": ".amdhsa_next_free_vgpr",
    "sgpr": ".amdhsa_next_free_sgpr",
    "scratch_bytes": ".amdhsa_private_segment_fixed_size",
    "lds_bytes": ".amdhsa_group_segment_fixed_size",
}


def parse(path):
    """key -> (normalised text, figures) for every kernel of one listing"""
    lines = open(path).read().splitlines()
    names = [l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")]
    keys = {n: kernel_key(d) for n, d in demangle(names).items()}
    assert len(set(keys.values())) == len(names), "kernel keys collide"
    token = re.compile(r"_Z[\w$.]+")

    def norm(text):
        text = token.sub(lambda m: keys.get(m.group(0), m.group(0)), text)
        return re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", text)

    # a kernel's text runs from its label to its .Lfunc_end; the .amdhsa_ block lies inside
    body = {}
    i = 0
    while i < len(lines):
        name = lines[i].split(":", 1)[0]
        if name in keys and lines[i].startswith(name + ":"):
            j = i
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            body[name] = lines[i:j]
            i = j
        i += 1
    out = {}
    for n in names:
        fig = {}
        for d in body[n]:
            f = d.split()
            for k, word in AMDHSA.items():
                if f and f[0] == word:
                    fig[k] = int(f[1])
        text = norm("\n".join(l for l in body[n] if "__hip_cuid_" not in l))
        out[keys[n]] = (text, {"vgpr": fig["accum_offset"],
                               "agpr": fig["next_free_vgpr"] - fig["accum_offset"],
                               "sgpr": fig["sgpr"], "scratch_bytes": fig["scratch_bytes"],
                               "lds_bytes": fig["lds_bytes"]})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("-o", "--out", help="write the per-kernel result as JSON")
    ap.add_argument("--show", type=int, default=10, help="differing kernels to name")
    a = ap.parse_args()
    old, new = parse(a.parent), parse(a.new)
    kernels = {}
    for k in sorted(set(old) | set(new)):
        o, n = old.get(k), new.get(k)
        kernels[k] = {"identical": bool(o and n and o[0] == n[0]),
                      "parent": o[1] if o else None, "new": n[1] if n else None}
    bwd = [k for k in kernels if k.startswith("bwd_rt_kernel ")]
    diff = [k for k, v in kernels.items() if not v["identical"]]
    summary = {
        "kernels_parent": len(old), "kernels_new": len(new), "same_kernel_set": set(old) == set(new),
        "backward_kernels": len(bwd),
        "backward_identical": sum(kernels[k]["identical"] for k in bwd),
        "other_kernels": len(kernels) - len(bwd),
        "other_identical": sum(v["identical"] for k, v in kernels.items() if k not in bwd),
    }
    print(json.dumps(summary, indent=1))
    for k in diff[:a.show]:
        print("differs:", k, kernels[k]["parent"], kernels[k]["new"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"summary": summary, "kernels": kernels}, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0 if summary["same_kernel_set"] and not diff else 1


if __name__ == "__main__":
    sys.exit(main())

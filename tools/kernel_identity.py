#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device-assembly listings of one csrc/*.hip file.

The check behind a refactor that must not change the machine code, or may only reorder it.
Needs no GPU. Compile the parent's and the new source with the Makefile's flags for that
object plus `--cuda-device-only -S`, e.g. for field_fused.o:

    hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -fno-honor-nans -mno-amdgpu-ieee \
          -mllvm -amdgpu-mfma-vgpr-form=1 -mllvm -amdgpu-sched-strategy=max-ilp \
          --cuda-device-only -S field_fused.hip -o side.s

    tools/kernel_identity.py --names field parent.s new.s -o profiles/field_bwd_refactor.json
    tools/kernel_identity.py --names hashgrid parent.s new.s -o out.json

Per kernel the text from its label to its end, .amdhsa_ block included, is compared as one
string, after every mangled kernel name has been replaced by a neutral key and the function
numbers of local labels have been dropped. --names selects the map from a parent's positional
template arguments to today's named forms, so that both spellings give the same key:
`field` for the field backward kernel, `hashgrid` for the hash-grid kernels (hashgrid.hip and
the hash + field kernels of field_fused.hip). Per kernel it also reports the instruction
count of both sides and whether the opcode multisets are equal (a kernel that differs with
equal multisets is a pure reordering; where they differ, the opcodes whose counts differ),
next to the .amdhsa_ register, scratch and LDS figures (vgpr: the accumulation offset, i.e.
the architectural VGPRs rounded up to 4; agpr: what follows it; vgpr_total: next_free_vgpr, the
figure that sets the waves per SIMD). Exit status 0: same kernels, all identical.

profiles/field_bwd_refactor.json was written by this tool's first form: run on the same two
listings with --names field, today's output has the same kernel keys, verdicts, register
figures and summary counts, plus the keys added since (instructions, same_opcodes, opcode_delta,
vgpr_total; identical / reordered / changed / only_* in the summary).
"""
import argparse
import collections
import json
import re
import subprocess
import sys

# field: parent spelling bwd_rt_kernel<W, NHD, FAST, ROWS, BF, REF, HG, S>:
# (FAST, ROWS, REF, HG) -> form
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


def split_args(args):
    return [p.strip() for p in re.split(r",\s*(?![^<]*>)", args)]


def field_key(demangled):
    m = re.search(r"bwd_rt_kernel<(.*)>\(anr::field::Args", demangled)
    if not m:
        return demangled
    parts = split_args(m.group(1).replace("anr::field::", ""))
    if len(parts) == 8:  # the parent's positional flags
        w, nhd, fast, rows, bf, ref, hg, s = parts
        form = old_form(fast, rows, ref, hg)
    else:
        w, nhd, bf, s, form = parts
    return "bwd_rt_kernel W=%s NHD=%s %s S=%s %s" % (w, nhd, "bf16" if bf == "true" else "f16", s, form)


def old_walk(xs, ds, count, bsz, sparse):
    """hashgrid_bwd_v2_kernel<D, TG, XS, DS, COUNT, BSZ, SPARSE> -> the walk type"""
    if sparse == "true":
        return "RowBitsWalk"
    if count == "true":
        return "CountRequests"
    if bsz == "8":
        return "TileMaskWalk"
    return "DenseWalk<%s, %s>" % (xs, ds)


def hashgrid_key(demangled):
    name = demangled.split("(")[0]
    m = re.search(r"hashgrid_bwd_v2_kernel<(.*)>$", name)
    if m:
        parts = split_args(m.group(1).replace("anr::", ""))
        walk = old_walk(*parts[2:]) if len(parts) == 7 else parts[2]
        return "hashgrid_bwd_v2_kernel D=%s %s %s" % (parts[0], parts[1], walk)
    # the run-leader cap left the kernels' template arguments (64 for the planes, 0 for the
    # hash + field forward and the render kernel)
    m = re.search(r"(hashgrid_fwd_planes_kernel)<(\d), (\w+)(, 64)?>$", name)
    if m:
        return "%s<%s, %s>" % m.group(1, 2, 3)
    m = re.search(r"(hf_fwd_kernel|render_kernel)<(.*)>$", name)
    if m:
        parts = split_args(m.group(2))
        n = 5 if m.group(1) == "hf_fwd_kernel" else 6
        assert len(parts) == n or (len(parts) == n + 1 and parts[n] == "0"), name
        return "%s<%s>" % (m.group(1), ", ".join(parts[:n]))
    return demangled


NAME_MAPS = {"field": field_key, "hashgrid": hashgrid_key}


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


def opcodes(body):
    """opcode -> count over a kernel's instruction lines"""
    ops = collections.Counter()
    for l in body:
        t = l.strip()
        if t and t[0] not in ".;" and not t.split(";")[0].rstrip().endswith(":"):
            ops[t.split()[0]] += 1
    return ops


def parse(path, kernel_key):
    """key -> (normalised text, figures, opcode counts) for every kernel of one listing"""
    lines = open(path).read().splitlines()
    names = [l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel ")]
    keys = {n: kernel_key(d) for n, d in demangle(names).items()}
    assert len(set(keys.values())) == len(names), "kernel keys collide"
    token = re.compile(r"_Z[\w$.]+")

    def norm(text):
        text = token.sub(lambda m: keys.get(m.group(0), m.group(0)), text)
        text = re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1", text)
        return re.sub(r"=BB\d+_", "=BB_", text)  # the loop-header comments name blocks too

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
                               "vgpr_total": fig["next_free_vgpr"],
                               "sgpr": fig["sgpr"], "scratch_bytes": fig["scratch_bytes"],
                               "lds_bytes": fig["lds_bytes"]}, opcodes(body[n]))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("parent")
    ap.add_argument("new")
    ap.add_argument("--names", choices=sorted(NAME_MAPS), default="field",
                    help="the old positional -> new named template-argument map")
    ap.add_argument("-o", "--out", help="write the per-kernel result as JSON")
    ap.add_argument("--show", type=int, default=10, help="differing kernels to name")
    a = ap.parse_args()
    old, new = parse(a.parent, NAME_MAPS[a.names]), parse(a.new, NAME_MAPS[a.names])
    kernels = {}
    for k in sorted(set(old) | set(new)):
        o, n = old.get(k), new.get(k)
        kernels[k] = {"identical": bool(o and n and o[0] == n[0]),
                      "parent": o[1] if o else None, "new": n[1] if n else None,
                      "instructions": {"parent": sum(o[2].values()) if o else None,
                                       "new": sum(n[2].values()) if n else None},
                      "same_opcodes": bool(o and n and o[2] == n[2])}
        if o and n and o[2] != n[2]:  # opcode -> [parent, new] where the counts differ
            kernels[k]["opcode_delta"] = {op: [o[2][op], n[2][op]]
                                          for op in sorted(set(o[2]) | set(n[2]))
                                          if o[2][op] != n[2][op]}
    diff = [k for k, v in kernels.items() if not v["identical"]]
    summary = {
        "kernels_parent": len(old), "kernels_new": len(new), "same_kernel_set": set(old) == set(new),
        "identical": len(kernels) - len(diff),
        "reordered": sum(kernels[k]["same_opcodes"] for k in diff),
        # in both listings, with other opcode counts; a kernel of one listing only is counted apart
        "changed": sum(not kernels[k]["same_opcodes"] for k in diff if k in old and k in new),
        "only_parent": len(set(old) - set(new)), "only_new": len(set(new) - set(old)),
    }
    if a.names == "field":
        bwd = [k for k in kernels if k.startswith("bwd_rt_kernel ")]
        summary.update({
            "backward_kernels": len(bwd),
            "backward_identical": sum(kernels[k]["identical"] for k in bwd),
            "other_kernels": len(kernels) - len(bwd),
            "other_identical": sum(v["identical"] for k, v in kernels.items() if k not in bwd),
        })
    print(json.dumps(summary, indent=1))
    for k in diff[:a.show]:
        v = kernels[k]
        print("reordered:" if v["same_opcodes"] else "differs:", k, v["parent"], v["new"],
              v["instructions"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"summary": summary, "kernels": kernels}, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0 if summary["same_kernel_set"] and not diff else 1


if __name__ == "__main__":
    sys.exit(main())

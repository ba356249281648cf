"""A/B of the hash-grid backward generations at bench size (profiling aid).

    python tools/hash_bwd_ab.py [--modes 0,1] [--iters 10] [--grad f16] [--rows] [--dims 2]

Bench coordinates (synthetic HARP2 scene -> fused sampler, 8192 rays x 1024 samples), f32
(or f16) dL/denc, f32 gradient table; --rows: anr_hashgrid_bwd_rows with ~70 % of the rows
zero in runs and the bits of the nonzero rows (the row-bits walk). Prints the HIP-event average per mode and the relative L2
difference of each mode's gradient from the first mode's. (The r02 log's mode 8, the
segment-flush backward v3, was removed from the library after measuring it.)
"""

from __future__ import annotations

import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "atmospheric-neural-rendering_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from atmonr_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--modes", default="0,1")
    ap.add_argument("--grad", choices=["f32", "f16"], default="f32")
    ap.add_argument("--rows", action="store_true")
    ap.add_argument("--dims", type=int, choices=[2, 3], default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B, N = args.rays, args.samples
    M = B * N
    from atmonr_amd.batch_loader import BatchLoader
    from atmonr_amd.datasets.synthetic import SyntheticHARP2Dataset
    from atmonr_amd.samplers import sample_and_preprocess

    ds = SyntheticHARP2Dataset(n_views=8, img_size=512, device=dev, seed=0)
    batch = next(iter(BatchLoader(ds, B, shuffle=True, seed=0)))
    prep = ds.get_point_preprocessor("horizontal").params(ngp_remap=True, alt_compress=8.0)
    _, _, coords = sample_and_preprocess(batch, N, prep)
    D = args.dims  # 2: the first two coordinates, rows of 2 (the run-time-stride form)
    x = coords.reshape(M, 3)[:, :D].contiguous()
    desc = _lib.hashgrid_desc(D, 16, 2, 16, 1.3819, 19)
    denc = torch.randn(M, 32, device=dev) * 1e-3
    gdt = _lib.F32
    if args.grad == "f16":
        denc, gdt = denc.half(), _lib.F16
    extra, entry = (), "anr_hashgrid_bwd"
    if args.rows:
        zero = (torch.rand(-(-M // 8), device=dev) < 0.5).repeat_interleave(8)[:M]
        denc[zero | (torch.rand(M, device=dev) < 0.4)] = 0.0
        nz = torch.nn.functional.pad((denc != 0).any(1).to(torch.int64), (0, -M % 32)).view(-1, 32)
        w = (nz << torch.arange(32, device=dev)[None]).sum(1)
        bits = torch.where(w >= 2**31, w - 2**32, w).to(torch.int32)
        extra, entry = (bits.data_ptr(),), "anr_hashgrid_bwd_rows"
    lib = _lib.load()
    s = _lib.stream(dev)
    grads = {}
    for mode in [int(m) for m in args.modes.split(",")]:
        grad = torch.zeros(desc.n_params, device=dev)
        prev = lib.anr_hashgrid_force_v1(mode)
        timer = _lib.KernelTimer()
        for it in range(args.iters + 2):
            if it == 2:
                timer.__enter__()
            if it == args.iters + 1:
                grad.zero_()
            _lib.call(entry, ctypes.byref(desc), x.data_ptr(), D, M, denc.data_ptr(), gdt, 32,
                      grad.data_ptr(), *extra, s, tag=f"hash_bwd_m{mode}")
        timer.__exit__(None, None, None)
        torch.cuda.synchronize()
        lib.anr_hashgrid_force_v1(prev)
        for k, v in timer.summary().items():
            print(f"mode {mode}: {k} avg {v['avg_ms']:.4f} ms ({v['launches']} calls)", flush=True)
        grads[mode] = grad
    first = next(iter(grads.values()))
    for m, g in grads.items():
        rel = ((g - first).norm() / first.norm().clamp_min(1e-30)).item()
        print(f"mode {m}: rel L2 vs first {rel:.3e}", flush=True)


if __name__ == "__main__":
    main()

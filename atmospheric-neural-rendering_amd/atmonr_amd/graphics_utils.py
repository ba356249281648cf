"""Volume rendering — same API as src/atmonr/graphics_utils.py:6-77, on the K8 kernels.

``render(z_vals, color, sigma)`` and ``render_with_surface(z_vals, color, sigma,
color_surf)`` return exactly the reference's tuples. Both are differentiable w.r.t.
color, sigma, color_surf and z_vals (the NeRF fine pass back-propagates into z through
sample_pdf). Arithmetic is f32 inside the kernel for any storage dtype; the outputs
have ``color.dtype`` as in the reference (graphics_utils.py:28).

``voxel_traversal(u, end)`` (graphics_utils.py:80-147) returns the voxels a set of segments
passes through: an exact f64 walk into a bitmap (csrc/voxels.hip) and the bitmap's ordered
compaction. :class:`VoxelBitmap` is the bitmap itself, for callers that feed it chunks of rays.
"""

from __future__ import annotations

import torch

from . import _lib
from ._lib import ANRError, call, dtype_code, ptr


class _CompositeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, color, sigma, color_surf, z_scale: float, want_alpha: bool):
        B, N, C = color.shape
        S = sigma.shape[2]
        dt = color.dtype
        dev = color.device
        sigma = sigma.to(dt).contiguous()
        color = color.contiguous()
        cs = color_surf.to(dt).contiguous() if color_surf is not None else None
        zc = z.float().contiguous()
        color_map = torch.empty(B, C, device=dev, dtype=dt)
        atmo = torch.empty(B, C, device=dev, dtype=dt) if cs is not None else None
        surf = torch.empty(B, C, device=dev, dtype=dt) if cs is not None else None
        weights = torch.empty(B, N, S, device=dev, dtype=dt)
        alpha = torch.empty(B, N, S, device=dev, dtype=dt)
        call("anr_composite_fwd", ptr(zc), float(z_scale), ptr(color), ptr(sigma), ptr(cs),
             dtype_code(dt), B, N, C, S, ptr(color_map), ptr(atmo), ptr(surf), ptr(weights),
             ptr(alpha), _lib.stream(dev))
        ctx.save_for_backward(zc, color, sigma, cs)
        # outputs the loss does not use (alpha, weights, atmo, surf in training) arrive as
        # None instead of materialised zero tensors: the kernel skips null gradients
        ctx.set_materialize_grads(False)
        ctx.z_scale = float(z_scale)
        ctx.has_surf = cs is not None
        ctx.z_dtype = z.dtype
        if cs is None:
            return color_map, alpha, weights
        return color_map, alpha, weights, atmo, surf

    @staticmethod
    def backward(ctx, *grads):
        zc, color, sigma, cs = ctx.saved_tensors
        B, N, C = color.shape
        S = sigma.shape[2]
        dt = color.dtype
        dev = color.device
        if ctx.has_surf:
            g_cm, g_alpha, g_w, g_atmo, g_surf = grads
        else:
            g_cm, g_alpha, g_w = grads
            g_atmo = g_surf = None

        def prep(g):
            return None if g is None else g.to(dt).contiguous()

        if g_cm is None:  # the kernel requires dL/dcolor_map
            g_cm = torch.zeros(B, color.shape[2], device=dev, dtype=dt)

        need_z, need_c, need_s, need_cs = ctx.needs_input_grad[:4]
        d_color = torch.empty_like(color) if need_c else None
        d_sigma = torch.empty_like(sigma) if need_s else None
        d_cs = torch.empty_like(cs) if (need_cs and cs is not None) else None
        d_z = torch.empty(B, N, device=dev, dtype=torch.float32) if need_z else None
        args = (ptr(zc), ctx.z_scale, ptr(color), ptr(sigma), ptr(cs), dtype_code(dt), B, N, C,
                S, ptr(prep(g_cm)), ptr(prep(g_atmo)), ptr(prep(g_surf)), ptr(prep(g_w)),
                ptr(prep(g_alpha)), ptr(d_color), ptr(d_sigma), ptr(d_cs), ptr(d_z))
        call("anr_composite_bwd", *args, _lib.stream(dev))
        if d_z is not None:
            d_z = d_z.to(ctx.z_dtype)
        return d_z, d_color, d_sigma, d_cs, None, None


class _CompositeRef16Fn(torch.autograd.Function):
    """render_with_surface with the reference's f16 numerics (anr_composite_ref16_*)."""

    @staticmethod
    def forward(ctx, z, color, sigma, color_surf, z_scale: float, zero_rays, want16: bool,
                need_alpha: bool, park: bool):
        B, N, C = color.shape
        if sigma.shape[2] != 1:
            raise ANRError("reference-numerics composite: one density channel (B, N, 1)")
        dev = color.device
        color, sigma = color.contiguous(), sigma.contiguous()
        cs = color_surf.to(color.dtype).contiguous() if color_surf is not None else None
        zc = z.float().contiguous()
        f16 = torch.float16
        cm = torch.empty(B, C, device=dev, dtype=f16)
        atmo = torch.empty(B, C, device=dev, dtype=f16)
        surf = torch.empty(B, C, device=dev, dtype=f16) if cs is not None else None
        weights = torch.empty(B, N, 1, device=dev, dtype=f16)
        alpha = torch.empty(B, N, 1, device=dev, dtype=f16) if need_alpha else None
        # f16 inputs hold the f16 values already: no copies are written, the inputs themselves
        # are saved for the backward and returned as the f16 colour / density results
        copies = want16 and color.dtype != f16
        c16 = torch.empty(B, N, C, device=dev, dtype=f16) if copies else None
        s16 = torch.empty(B, N, 1, device=dev, dtype=f16) if copies else None
        args = (ptr(zc), float(z_scale), ptr(color), ptr(sigma), ptr(cs),
                dtype_code(color.dtype), B, N, C, ptr(cm), ptr(atmo), ptr(surf), ptr(weights),
                ptr(alpha), ptr(c16), ptr(s16))
        if park:
            # a backward will follow on these same tensors: the kernel also leaves it T_i and
            # exp(-sigma_i delta_i) (one 4-byte pair per sample) and, per ray, the surface
            # product and the alpha-is-1 flag, so the backward does not replay the forward
            pk = torch.empty(B, N, device=dev, dtype=torch.int32)
            rpk = torch.empty(B, device=dev, dtype=torch.int32)
            call("anr_composite_ref16_fwd_park", *args, ptr(pk), ptr(rpk), _lib.stream(dev),
                 tag="composite_fwd")
        else:
            pk = rpk = None
            call("anr_composite_ref16_fwd", *args, _lib.stream(dev), tag="composite_fwd")
        # the backward reads the inputs as f16 values either way: with the f16 copies at
        # hand it reads those (half the bytes of f32 inputs) and still returns gradients in
        # the inputs' dtype
        ctx.out_dtype = color.dtype
        ctx.parked = park
        if copies:
            ctx.save_for_backward(zc, c16, s16, cs, pk, rpk)
        else:
            ctx.save_for_backward(zc, color, sigma, cs, pk, rpk)
            if want16:
                c16, s16 = color.detach(), sigma.detach()
        ctx.set_materialize_grads(False)
        ctx.z_scale = float(z_scale)
        ctx.zero_rays = zero_rays
        outs = (cm, alpha, weights) if cs is None else (cm, alpha, weights, atmo, surf)
        if want16:
            ctx.mark_non_differentiable(c16, s16)
            outs = outs + (c16, s16)
        return outs

    @staticmethod
    def backward(ctx, g_cm, *unused):
        zc, color, sigma, cs, pk, rpk = ctx.saved_tensors
        if any(g is not None for g in unused):
            raise ANRError("reference-numerics composite: gradients flow through color_map "
                           "only (as in the reference's loss)")
        B, N, C = color.shape
        dev = color.device
        if g_cm is None:
            g_cm = torch.zeros(B, C, device=dev, dtype=torch.float16)
        g_cm = g_cm.to(torch.float16).contiguous()
        od = ctx.out_dtype
        d_color = torch.empty(color.shape, device=dev, dtype=od)
        d_sigma = torch.empty(sigma.shape, device=dev, dtype=od)
        d_cs = (torch.empty(cs.shape, device=dev, dtype=od)
                if cs is not None and ctx.needs_input_grad[3] else None)
        if cs is not None and cs.dtype != color.dtype:
            cs = cs.to(color.dtype)
        args = (ptr(zc), ctx.z_scale, ptr(color), ptr(sigma), ptr(cs), dtype_code(color.dtype),
                B, N, C, ptr(g_cm), ptr(d_color), ptr(d_sigma), ptr(d_cs), dtype_code(od),
                ptr(ctx.zero_rays))
        if pk is not None:
            call("anr_composite_ref16_bwd_parked", *args, ptr(pk), ptr(rpk), _lib.stream(dev),
                 tag="composite_bwd")
        else:
            call("anr_composite_ref16_bwd", *args, _lib.stream(dev), tag="composite_bwd")
        return None, d_color, d_sigma, d_cs, None, None, None, None, None


def render_with_surface_ref16(z_vals, color, sigma, color_surf, z_scale: float = 1.0,
                              zero_rays: torch.Tensor | None = None, inputs_f16: bool = False,
                              need_alpha: bool = True):
    """graphics_utils.py:52-77 with the reference's Instant-NGP numerics: z cast to f16
    (after the f32 ``z_vals * z_scale``), every op rounded to f16, torch's CUDA
    accumulation (f16 cumprod / cumsum, f32 sum / prod), and torch's f16 autograd as the
    backward (csrc/ref16.hip; restated in oracle/ref_f16.py). color / sigma / color_surf
    may be f32 (rounded to f16 on load, as a tcnn f16 output would be). Returns f16
    (color_map, alpha, weights, atmo, surf). ``zero_rays`` (int32 device tensor, optional)
    counts rays whose alpha rounded to exactly 1 in f16 (torch's zero-input backward
    branch, not reproduced: those rays get zero gradients). ``inputs_f16``: also return
    color and sigma rounded to f16 as the kernel reads them (tcnn's f16 outputs, which the
    reference's forward returns), written by the same kernel; f16 color / sigma are returned
    as they are (no copy). f16 inputs also get f16 gradients, and the backward then parks its
    two scratch values per sample as one 4-byte pair (csrc/ref16.hip). ``need_alpha=False``:
    alpha is not written and its slot of the result is None. When a gradient can flow
    (grad mode on and color, sigma or color_surf requires grad) the forward also parks T,
    exp(-sigma delta) and the surface product for its backward (4 bytes per sample, held
    until the backward ran), which then skips its replay of the forward; an inference
    forward writes no park."""
    _check(z_vals, color, sigma)
    if zero_rays is None:
        zero_rays = torch.zeros(1, dtype=torch.int32, device=color.device)
    park = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (color, sigma, color_surf))
    return _CompositeRef16Fn.apply(z_vals, color, sigma, color_surf, z_scale, zero_rays,
                                   bool(inputs_f16), bool(need_alpha), park)


def _check(z_vals, color, sigma):
    if not (z_vals.dim() == 2 and color.dim() == 3 and sigma.dim() == 3):
        raise ANRError("render: expected z (B,N), color (B,N,C), sigma (B,N,S)")
    if z_vals.shape != color.shape[:2] or z_vals.shape != sigma.shape[:2]:
        raise ANRError("render: z / color / sigma shapes disagree")
    if color.dtype not in (torch.float16, torch.float32):
        raise ANRError(f"render: unsupported dtype {color.dtype}")


def render(z_vals: torch.Tensor, color: torch.Tensor, sigma: torch.Tensor, z_scale: float = 1.0):
    """graphics_utils.py:6-49. Returns (color_map, alpha, weights).

    ``z_scale`` multiplies z in f32 inside the kernel (the pipelines pass scale/1000
    here instead of materialising z_vals*(scale/1000), instant_ngp.py:188).
    """
    _check(z_vals, color, sigma)
    return _CompositeFn.apply(z_vals, color, sigma, None, z_scale, True)


def render_with_surface(z_vals, color, sigma, color_surf, z_scale: float = 1.0):
    """graphics_utils.py:52-77. Returns (color_map, alpha, weights, atmo, surf)."""
    _check(z_vals, color, sigma)
    return _CompositeFn.apply(z_vals, color, sigma, color_surf, z_scale, True)


DEFAULT_MAX_BITMAP_BYTES = 4 << 30


class VoxelBitmap:
    """One bit per voxel of the box ``lo <= (i, j, k) <= hi`` (inclusive int corners), i
    fastest, rows padded to whole uint32 words (include/anr.h, "Global-grid extract").
    :meth:`add` ORs the voxels of a chunk of rays into it; :meth:`voxels` compacts it."""

    def __init__(self, lo, hi, device, max_bitmap_bytes: int = DEFAULT_MAX_BITMAP_BYTES):
        self.lo = tuple(int(v) for v in lo)
        self.ext = tuple(int(h) - int(l) + 1 for l, h in zip(lo, hi))
        if min(self.ext) < 1:
            raise ValueError(f"voxel box {self.lo} .. {tuple(hi)} is empty")
        self.row_pitch = (self.ext[0] + 31) // 32 * 32
        self.n_words = self.row_pitch // 32 * self.ext[1] * self.ext[2]
        if self.n_words * 4 > max_bitmap_bytes:
            raise ValueError(
                f"voxel box of {self.ext[0]} x {self.ext[1]} x {self.ext[2]} voxels from "
                f"{self.lo} needs a bitmap of {self.n_words * 4} bytes, above the limit of "
                f"{max_bitmap_bytes} bytes (max_bitmap_bytes)")
        self.device = torch.device(device)
        # int32 storage (torch has no uint32 arithmetic); the kernels see uint32 words
        self.words = torch.zeros(self.n_words, dtype=torch.int32, device=self.device)
        self.counters = torch.zeros(2, dtype=torch.int64, device=self.device)

    @staticmethod
    def bounds(u: torch.Tensor, end: torch.Tensor):
        """Inclusive int corners of the floored endpoints of the rays whose two endpoints are
        finite (``amin`` / ``amax``, a few million rays at a time), or None without any."""
        lo = hi = None
        for s in range(0, u.shape[0], 1 << 22):
            pts = torch.stack([u[s:s + (1 << 22)], end[s:s + (1 << 22)]], dim=1).double()
            pts = torch.floor(pts[torch.isfinite(pts).all(dim=2).all(dim=1)]).reshape(-1, 3)
            if pts.shape[0] == 0:
                continue
            clo, chi = pts.amin(dim=0), pts.amax(dim=0)
            lo = clo if lo is None else torch.minimum(lo, clo)
            hi = chi if hi is None else torch.maximum(hi, chi)
        if lo is None:
            return None
        lo, hi = lo.tolist(), hi.tolist()
        if max(abs(v) for v in lo + hi) >= 2.0 ** 31 - 1:
            raise ValueError(f"voxel coordinates {lo} .. {hi} do not fit int32")
        return [int(v) for v in lo], [int(v) for v in hi]

    def add(self, u: torch.Tensor, end: torch.Tensor, shortcut: bool = True) -> None:
        if u.shape != end.shape or u.dim() != 2 or u.shape[1] != 3:
            raise ANRError("voxel traversal: u and end must both be (R, 3)")
        u = u.to(device=self.device, dtype=torch.float64).contiguous()
        end = end.to(device=self.device, dtype=torch.float64).contiguous()
        call("anr_voxel_traverse", ptr(u), ptr(end), u.shape[0], *self.lo, *self.ext,
             self.row_pitch, ptr(self.words), ptr(self.counters), int(bool(shortcut)),
             _lib.stream(self.device))

    def skipped_rays(self) -> int:
        """Rays that marked nothing because an endpoint was not finite."""
        return int(self.counters[0].item())

    def voxels(self) -> torch.Tensor:
        """(n, 3) int32 (i, j, k) of the set bits in ascending bitmap order (k slowest, i
        fastest). Raises when a ray had a voxel outside the box."""
        outside = int(self.counters[1].item())
        if outside:
            raise ANRError(f"voxel traversal: {outside} voxels of rays that leave the box "
                           f"{self.lo} + {self.ext} were not marked")
        st = _lib.stream(self.device)
        n_blocks = _lib.load().anr_voxel_n_blocks(self.n_words)
        counts = torch.empty(n_blocks, dtype=torch.int32, device=self.device)
        call("anr_voxel_count", ptr(self.words), *self.ext, self.row_pitch, ptr(counts), st)
        ends = torch.cumsum(counts, dim=0, dtype=torch.int64)
        offsets = (ends - counts).contiguous()
        n = int(ends[-1].item())
        out = torch.empty((n, 3), dtype=torch.int32, device=self.device)
        call("anr_voxel_compact", ptr(self.words), *self.lo, *self.ext, self.row_pitch,
             ptr(offsets), n, ptr(out), st)
        return out


def voxel_traversal(u: torch.Tensor, end: torch.Tensor, unique_only: bool = True,
                    max_bitmap_bytes: int = DEFAULT_MAX_BITMAP_BYTES) -> torch.Tensor:
    """graphics_utils.py:80-147: all voxels (edge 1) that the segments ``u -> end`` pass
    through. ``u``, ``end``: GPU tensors (R, 3) of any float dtype, widened to f64. Returns
    the unique voxels as (n, 3) int32, sorted with k slowest and i fastest -- the same for any
    order or chunking of the rays and from run to run.

    The walk is exact in f64 (csrc/voxels.hip): the reference accumulates its crossing times
    in the input's precision and can leave the true path at large coordinates; its indices
    are int16, these int32. ``unique_only=False`` returns the same tensor: the voxels are
    collected in a bitmap, which has no duplicates. Rays with a non-finite endpoint are
    skipped. The bitmap spans the bounding box of the floored endpoints; a box that needs
    more than ``max_bitmap_bytes`` raises ValueError (the box is not tiled)."""
    if not (u.is_cuda and end.is_cuda):
        raise ANRError("voxel_traversal needs GPU tensors (got a CPU tensor)")
    if u.shape != end.shape or u.dim() != 2 or u.shape[1] != 3:
        raise ANRError("voxel_traversal: u and end must both be (R, 3)")
    box = VoxelBitmap.bounds(u, end)
    if box is None:
        return torch.empty((0, 3), dtype=torch.int32, device=u.device)
    bitmap = VoxelBitmap(box[0], box[1], u.device, max_bitmap_bytes)
    bitmap.add(u, end)
    return bitmap.voxels()

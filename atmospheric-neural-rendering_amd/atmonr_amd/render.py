"""Rendering rays to colour maps without a backward: a whole view, a held-out view, the
PSNR checkpoints of a run (trainer.py:150-170), an image after loading a checkpoint.

``render_rays`` loops an unshuffled ``BatchLoader`` over a dataset's rays, all of them or
the rays ``idx``, and calls ``pipeline.render`` on every batch: for an Instant-NGP pipeline
whose configuration anr_ingp_render takes that is one kernel per batch for the hash grid,
the field and the composite, with no per-sample tensor but the sampler's coordinates and z
(16 B per sample, where the training forward holds over 200 B per sample for its backward);
every other pipeline runs its forward under ``no_grad``. ``render_images`` turns the maps
into the (V, H, W) cube of the dataset's views and its image metrics (harp2.py:297-335).
The host only slices index ranges.
"""

from __future__ import annotations

import torch

from .batch_loader import BatchLoader

MAPS = ("color_map_fine", "color_map_atmo", "color_map_surf")


class _RaySubset:
    """The rays ``idx`` of a dataset, as a dataset for BatchLoader."""

    def __init__(self, dataset, idx: torch.Tensor) -> None:
        self.dataset = dataset
        self.idx = idx
        self.device = getattr(dataset, "device", idx.device)

    def __len__(self) -> int:
        return int(self.idx.shape[0])

    def __getbatch__(self, i: torch.Tensor) -> dict[str, torch.Tensor]:
        return self.dataset.__getbatch__(self.idx[i])


def render_rays(pipeline, dataset, idx: torch.Tensor | None = None, batch_size: int = 8192,
                **render_kw) -> dict[str, torch.Tensor]:
    """``pipeline.render`` over the rays of ``dataset`` (``idx``: those rays, in that order;
    default all), ``batch_size`` rays at a time, in order. Returns the (R, num_bands) maps
    ``color_map_fine``, ``color_map_atmo`` and ``color_map_surf`` (those the pipeline's
    render returns). Rays are independent, so the batch size does not change a value.
    ``render_kw`` goes to ``pipeline.render`` (``fused=``, ``random=``)."""
    src = dataset if idx is None else _RaySubset(dataset, idx)
    loader = BatchLoader(src, batch_size=batch_size, shuffle=False)
    out: dict[str, torch.Tensor] = {}
    for (s, e), batch in zip(loader.slices(), loader):
        res = pipeline.render(batch, **render_kw)
        for k in MAPS:
            if k not in res:
                continue
            if k not in out:
                out[k] = torch.empty((len(src),) + tuple(res[k].shape[1:]), dtype=res[k].dtype,
                                     device=res[k].device)
            out[k][s:e] = res[k]
    return out


def render_images(pipeline, dataset, batch_size: int = 8192, **render_kw):
    """Every ray of ``dataset`` rendered and scattered into its views: returns the predicted
    (V, H, W) cube -- each ray's colour at its own band ``irgb_idx``, as ``compute_loss``
    picks it (instant_ngp.py:259-261) -- and ``dataset.get_image_metrics(pred,
    dataset.target_image())``."""
    src_loader = BatchLoader(dataset, batch_size=batch_size, shuffle=False)
    pix = None
    for (s, e), batch in zip(src_loader.slices(), src_loader):
        cm = pipeline.render(batch, **render_kw)["color_map_fine"]
        if pix is None:  # f32 pixels, whatever the maps' dtype (f16 in reference numerics)
            pix = torch.empty(len(dataset), dtype=torch.float32, device=cm.device)
        pix[s:e] = torch.take_along_dim(cm, batch["irgb_idx"][:, None], dim=1)[:, 0]
    pred = dataset.scatter_image(pix)
    return pred, dataset.get_image_metrics(pred, dataset.target_image())

"""Test-time augmentation for the CenterNet meta-architecture: CenterNet's flip test.

The reference's TEST.AUG switches (detectron2/config/defaults.py:634-638) drive `GeneralizedRCNNWithTTA`
(detectron2/modeling/test_time_augmentation.py), which asserts a GeneralizedRCNN; for CenterNet the reference holds
nothing.  What CenterNet's published numbers use is the flip test, and that is what `CenterNetWithTTA` runs:

  * the network runs on the input and on its horizontal mirror.  The mirror is taken on the NETWORK INPUT -- the normalised
    tensor after right/bottom zero padding to the size divisibility: mirrored image b has column x equal to column Wp-1-x
    of the plain one, so its zero padding sits on the left and the output maps are exact mirrors (x <-> W_out-1-x) for
    every image size, a multiple of 32 or not;
  * merged maps: hm = (hm[b] + mirror(hm[b+B])) * 0.5 on the sigmoid-and-clamped heat maps, wh = (wh[b] + mirror(wh[b+B]))
    * 0.5 -- one f32 add and one multiply by 0.5, in that order -- and reg = reg[b], the un-mirrored pass alone.  A mean of
    two clamped values still respects the clamp floor;
  * peak NMS, top-K, decode, thresholding and the per-image height / width rescale run once, on the merged maps of B
    images, exactly as without augmentation.

All of it happens inside the model's flip engine (meta_arch/centernet.py: _EvalEngine(flip=True)): the kernels that read
the images produce the mirrored half, the decode merges while it reads the maps, one captured graph per shape.

Multi-scale merging is not built: CenterNet merges scales by per-class soft-NMS, NMS ops are out of scope of this project
 and the reference has no CenterNet merge to pin one against.  More than one entry in
TEST.AUG.MIN_SIZES is refused at construction.
"""
import numpy as np
import torch

from ..data import transforms as T

__all__ = ["CenterNetWithTTA"]


class CenterNetWithTTA:
    """`CenterNetWithTTA(cfg, model)(batched_inputs)`: the model's `list[dict]` in, `[{"instances": Instances}]` out.

    TEST.AUG.FLIP: run the flip test (False: the plain path).  TEST.AUG.MIN_SIZES: () keeps the images as they come; one
    entry resizes every image with ResizeShortestEdge(size, TEST.AUG.MAX_SIZE) before the model, boxes come back in the
    frame of the original image through the inputs' `height` / `width` (the image's own size when absent)."""

    def __init__(self, cfg, model):
        from .meta_arch.centernet import CenterNet
        assert isinstance(model, CenterNet), (
            f"CenterNetWithTTA wraps this project's CenterNet meta-architecture, not {type(model).__name__}")
        sizes = tuple(cfg.TEST.AUG.MIN_SIZES)
        if len(sizes) > 1:
            raise NotImplementedError(
                f"TEST.AUG.MIN_SIZES={sizes}: multi-scale merging is not built (CenterNet merges scales by per-class "
                "soft-NMS; NMS ops are out of scope, DESIGN.md section 7, and the reference has no CenterNet merge to "
                "compare against). Give one size, or () to keep the input size.")
        self.cfg, self.model = cfg, model
        self.flip = bool(cfg.TEST.AUG.FLIP)
        self.resize = T.ResizeShortestEdge(int(sizes[0]), int(cfg.TEST.AUG.MAX_SIZE), "choice") if sizes else None

    # the parts of nn.Module that evaluation code touches (evaluation.inference_on_dataset)
    @property
    def training(self):
        return self.model.training

    def eval(self):
        self.model.eval()
        return self

    def train(self, mode=True):
        self.model.train(mode)
        return self

    def parameters(self):
        return self.model.parameters()

    def _inputs(self, batched_inputs):
        """the inputs at the test size, `height` / `width` pinned to the frame the boxes are wanted in"""
        if self.resize is None:
            return batched_inputs
        out = []
        for inp in batched_inputs:
            im = inp["image"]
            h, w = im.shape[-2:]
            new = dict(inp, height=inp.get("height", h), width=inp.get("width", w))
            if self.resize.output_size(h, w, self.resize.short_edge_length[0], self.resize.max_size) != (h, w):
                hwc = im.permute(1, 2, 0).cpu().numpy()
                tfm = self.resize.get_transform(hwc)
                new["image"] = torch.from_numpy(np.array(tfm.apply_image(hwc))).permute(2, 0, 1).contiguous()
            out.append(new)
        return out

    def _check(self):
        if self.model.training:
            raise RuntimeError("CenterNetWithTTA is an inference-time wrapper: call model.eval() first (no TTA in training)")

    def forward_async(self, batched_inputs):
        """a handle whose .result() is what __call__ returns (CenterNet.forward_async through the flip engine)"""
        self._check()
        return self.model.forward_async(self._inputs(batched_inputs), flip=self.flip)

    @torch.no_grad()
    def __call__(self, batched_inputs):
        self._check()
        return self.model._forward_eval(self._inputs(batched_inputs), flip=self.flip)

"""The (H, W) -> (new_h, new_w) cases of the resize tests (test_resize_host.py, test_resize_gpu.py), each with the reason it
is there, and the three images every case runs on."""
import numpy as np

COL_TILE = 64      # output columns of one block of csrc/resize.hip (RESIZE_TW); test_resize_host.py pins it to the source

# (name, (H, W), (new_h, new_w), what it is there for)
CASES = [
    ("up_down", (5, 7), (40, 3), "up in one axis, down in the other"),
    ("one_row", (1, 9), (4, 9), "one source row, horizontal pass skipped"),
    ("v_skipped", (64, 64), (64, 31), "vertical pass skipped"),
    ("one_pixel", (2, 2), (1, 1), "one-pixel output"),
    ("frac_down", (37, 53), (11, 7), "non-integer downscale, bounds clamped at both borders"),
    ("long_span", (3000, 17), (13, 17), "about 230 source rows per output row: no tile budget may bound the span"),
    ("pow2_plus1", (129, 257), (65, 129), "sizes one past a power of two"),
    ("partial_tile", (9, 50), (10, COL_TILE + 1), "new_w = the kernel's column tile + 1: a block with one live column"),
    ("workload", (480, 640), (512, 683), "the workload's own ratio"),
]
IMAGES = ("random", "checker", "white")


def make_image(kind, H, W, seed=0):
    """uint8 [H, W, 3]: random bytes; a 0/255 checkerboard (clipping and the rounding term); constant 255 (must stay 255:
    the coefficient sums round to 2**22)"""
    if kind == "random":
        return np.random.RandomState(seed).randint(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "checker":
        yy, xx = np.mgrid[0:H, 0:W]
        return np.ascontiguousarray((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None].repeat(3, 2))
    assert kind == "white", kind
    return np.full((H, W, 3), 255, dtype=np.uint8)


def all_inputs():
    """(id, image, (new_h, new_w)) for every case x image"""
    for i, (name, (H, W), new, _) in enumerate(CASES):
        for kind in IMAGES:
            yield f"{name}-{kind}", make_image(kind, H, W, seed=i), new

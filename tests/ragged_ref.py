"""What the tests of the batches of images of individual sizes (idc_forward_async_images) share: the size lists of the GPU file and the
arithmetic of the packed layout -- where each image starts in the slot's packed source and which images each 4-pixel group of the flat run
covers -- restated in numpy, so that the CPU file can show that the lists have the structure claimed for them."""
import numpy as np

import ingest_ref

# the mixed batch: every tap clamped, fewer pixels than a workgroup, up-scaling with 3 mod 4 bytes, the identity, down-scaling, several
# workgroups with a pixel count of 1 mod 4, and a six-pixel image at the end
MIXED = [(1, 1), (5, 7), (37, 41), "own", (130, 97), (203, 187), (2, 3)]
# groups that span many images (all with out='source')
FOUR_IN_ONE = [(1, 1), (1, 1), (1, 1), (5, 7)]                  # the first 4-pixel group covers four images
TAIL_IMAGE = [(5, 7), (1, 1), (1, 1)]                           # 37 pixels: the byte-access tail of the run is a 1 x 1 image of its own
THREE_BOUNDARIES = [(2, 3), (1, 2), (1, 1), (1, 3), (203, 187)]  # a group with three boundaries (start, inside, end), then a multi-workgroup image
SPANS = [FOUR_IN_ONE, TAIL_IMAGE, THREE_BOUNDARIES]


def sizes(lst, H, W):
    return [(H, W) if s == "own" else tuple(s) for s in lst]


def starts(sz):
    """Byte offset of every image in the packed source, and the total."""
    return np.concatenate([[0], np.cumsum([h * w * 3 for h, w in sz])]).astype(np.int64)


def image_of_pixel(sz):
    """Image index of every pixel of the flat run."""
    return np.repeat(np.arange(len(sz)), [h * w for h, w in sz])


def groups(sz):
    """(images of each full 4-pixel group [ngroups, 4], images of the total % 4 tail pixels)."""
    idx = image_of_pixel(sz)
    full = idx.size // 4 * 4
    return idx[:full].reshape(-1, 4), idx[full:]


_IMAGES = {}


def image(sh, sw, seed):
    """ingest_ref.source_image, made once per (size, seed) and never written to."""
    key = (sh, sw, seed)
    if key not in _IMAGES:
        a = np.ascontiguousarray(ingest_ref.source_image(sh, sw, seed))
        a.setflags(write=False)
        _IMAGES[key] = a
    return _IMAGES[key]

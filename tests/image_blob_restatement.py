"""The image blob in plain numpy, written from the rules and not from the code under test: per frame the host expression of the
detection loops, `(np.asarray(im, np.float64) - means).astype(np.float32)`, an optional left/right mirror of the frame within its own
width, and the padding rule of the reference's im_list_to_blob (lib/utils/blob.py:14-27) restated: a canvas of zeros with every frame
at its top-left corner."""
import numpy as np

PIXEL_MEANS = np.array([[[95.8814, 98.7743, 93.8549]]])          # cfg.PIXEL_MEANS (lib/fast_rcnn/config.py)


def frame(im, means=PIXEL_MEANS, flip=False):
    f = (np.asarray(im, np.float64) - means).astype(np.float32)
    return f[:, ::-1] if flip else f


def blob(images, canvas=None, means=PIXEL_MEANS, flip=None):
    """(B, H, W, 3) f32; canvas None = the frames' maximal height and width"""
    flip = [False] * len(images) if flip is None else list(flip)
    H, W = canvas if canvas is not None else (max(im.shape[0] for im in images), max(im.shape[1] for im in images))
    out = np.zeros((len(images), H, W, 3), np.float32)
    for b, im in enumerate(images):
        out[b, :im.shape[0], :im.shape[1]] = frame(im, means, flip[b])
    return out

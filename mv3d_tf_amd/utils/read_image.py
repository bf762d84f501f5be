"""The one image read of the test loops and the training minibatch (the reference uses cv2.imread; cv2 is not a dependency here)."""
import numpy as np


def read_image_bgr(path):
    """what cv2.imread returns, (h, w, 3) uint8 BGR: a `.npy` file through numpy, any other file through PIL as RGB, reversed"""
    if path.endswith(".npy"):
        return np.load(path)
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))[:, :, ::-1]

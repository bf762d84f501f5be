"""Image input on the device: ops.image_blob / mv3d_image_blob against image_blob_restatement (the host
expression of the loops per frame, an optional mirror, im_list_to_blob's padding), and the layers that build `image_data` from uint8
frames under cfg.IMAGE_BLOB_ON_DEVICE.  Every comparison is equality of the uint32 views, padding included; nothing has a tolerance.
Every device result is written into a buffer prefilled with NaN, so an element the kernel leaves out cannot pass."""
import ctypes as C

import numpy as np
import pytest

import image_blob_restatement as R

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def images(seed, shapes):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in shapes]


@pytest.fixture(scope="module")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops
    return {"torch": torch, "ops": ops}


def nan_frames(torch, shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def device_blob(gpu, ims, canvas=None, flip=None, **kw):
    """ops.image_blob on a list of images, into a NaN buffer of the shape the restatement gives -> host array"""
    want = R.blob(ims, canvas, flip=flip, **({"means": kw["means"]} if "means" in kw else {}))
    out = nan_frames(gpu["torch"], want.shape)
    got = gpu["ops"].image_blob(ims, canvas=canvas, flip=flip, out=out, **kw)
    assert got is out
    return got.cpu().numpy(), want


def _entry(**extra):
    e = {"image": images(5, [(8, 12)])[0], "lidar_bv": np.random.RandomState(0).random_sample((8, 601, 9)).astype(F32),
         "calib": np.arange(48, dtype=np.float64).reshape(4, 12), "gt_classes": np.array([1, 0], np.int32),
         "boxes": np.arange(8, dtype=F32).reshape(2, 4), "boxes_bv": np.arange(8, dtype=F32).reshape(2, 4) + 1,
         "boxes_3D": np.arange(12, dtype=F32).reshape(2, 6), "boxes_corners": np.arange(48, dtype=F32).reshape(2, 24), "flipped": False}
    e.update(extra)
    return e


# ---------------------------------------------------------------------------------------------------- CPU
def test_keys_default_off_and_nothing_changes():
    from mv3d_tf_amd.fast_rcnn import detect_batch
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    assert cfg.IMAGE_BLOB_ON_DEVICE is False and cfg.IMAGE_CANVAS is None
    entry = _entry()
    blobs = get_minibatch([entry], 2)
    assert set(blobs) == {"image_data", "lidar_bv_data", "calib", "gt_boxes", "gt_boxes_bv", "gt_boxes_3d", "gt_boxes_corners", "im_info"}
    assert all(isinstance(v, np.ndarray) for v in blobs.values())
    assert blobs["image_data"].dtype == F32 and blobs["image_data"].shape == (1, 8, 12, 3)
    assert np.array_equal(bits(blobs["image_data"]), bits((entry["image"].astype(F32) - cfg.PIXEL_MEANS).astype(F32)[None]))
    assert np.array_equal(blobs["lidar_bv_data"], entry["lidar_bv"][None]) and np.array_equal(blobs["im_info"], [[8, 601, 1]])
    # the loops' groups end at every change of image shape, as before
    ims = images(6, [(8, 12), (8, 12), (7, 11), (8, 13)])
    keys = [(detect_batch._image_key(im), (16, 16, 9)) for im in ims]
    assert keys[0][0] == (8, 12, 3) and detect_batch.group_frames(keys, 4) == [[0, 1], [2], [3]]
    cfg.IMAGE_BLOB_ON_DEVICE = True
    try:
        assert detect_batch.group_frames([(detect_batch._image_key(im), (16, 16, 9)) for im in ims], 4) == [[0, 1, 2, 3]]
    finally:
        cfg.IMAGE_BLOB_ON_DEVICE = False


def test_restatement_equals_both_host_expressions():
    from mv3d_tf_amd.fast_rcnn import detect_batch
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    assert np.array_equal(R.PIXEL_MEANS, cfg.PIXEL_MEANS)
    every = np.stack([np.arange(256, dtype=np.uint8).reshape(16, 16)] * 3, -1)          # every byte value in every channel
    ims = [every] + images(7, [(16, 16), (16, 16)])
    want = R.blob(ims)
    assert want.dtype == F32 and want.shape == (3, 16, 16, 3)
    assert np.array_equal(bits(want), bits(detect_batch.host_image_blob(ims)))                                  # test_net, imdb_proposals
    assert np.array_equal(bits(want), bits(np.stack([(np.asarray(im, np.float64) - cfg.PIXEL_MEANS).astype(F32) for im in ims])))
    for b, im in enumerate(ims):                                                                                # get_minibatch
        bev = np.zeros((4, 601, 9), F32)
        assert np.array_equal(bits(get_minibatch([_entry(image=im, lidar_bv=bev)], 2)["image_data"]), bits(want[b:b + 1]))
    # the premise of the every-value test: an f32 subtraction is NOT this expression
    assert (bits(every.astype(F32) - cfg.PIXEL_MEANS.astype(F32)) != bits(want[0])).sum() == 303 * 1
    # padding and mirror
    small = images(8, [(2, 3)])[0]
    padded = R.blob([small, ims[1]], flip=[True, False])
    assert padded.shape == (2, 16, 16, 3) and np.array_equal(padded[0, :2, :3], R.frame(small)[:, ::-1])
    assert not bits(padded[0, 2:]).any() and not bits(padded[0, :, 3:]).any()          # +0.0, the bit pattern 0


def test_pack_image_frames():
    from mv3d_tf_amd import ops
    ims = images(9, [(2, 3), (1, 1), (3, 2)])
    pixels, frames, shape = ops.pack_image_frames(ims)
    assert pixels.dtype == np.uint8 and pixels.shape == (18 + 3 + 18,) and pixels.flags["C_CONTIGUOUS"]
    assert frames.dtype == np.int32 and np.array_equal(frames, [[0, 2, 3, 0], [18, 1, 1, 0], [21, 3, 2, 0]]) and shape == (3, 3)
    for im, (o, h, w, _) in zip(ims, frames):
        assert np.array_equal(pixels[o:o + 3 * h * w].reshape(h, w, 3), im)
    view = np.ascontiguousarray(ims[0][:, ::-1])[:, ::-1]                                # a non-contiguous frame (what PIL's BGR is)
    assert not view.flags["C_CONTIGUOUS"] and np.array_equal(ops.pack_image_frames([view])[0], ims[0].reshape(-1))
    for exc, arg in ((TypeError, [ims[0].astype(F32)]), (TypeError, [ims[0].tolist()]), (ValueError, [ims[0][:, :, :2]]),
                     (ValueError, [ims[0][0]]), (ValueError, [np.zeros((0, 3, 3), np.uint8)]), (ValueError, [])):
        with pytest.raises(exc, match="pack_image_frames"):
            ops.pack_image_frames(arg)


def test_image_blob_refuses_bad_arguments_before_any_launch():
    import torch
    from mv3d_tf_amd import build
    build.build()
    from mv3d_tf_amd import ops
    px = np.zeros(30, np.uint8)
    tab = [[0, 2, 3, 0], [18, 1, 4, 0]]
    im = np.zeros((2, 3, 3), np.uint8)
    for exc, args, kw in ((TypeError, (px.astype(F32), tab), {}), (TypeError, (torch.zeros(30), tab), {}), (TypeError, (px, np.array(tab, F32)), {}),
                          (TypeError, (px, torch.zeros((2, 4), dtype=torch.int64)), {}), (TypeError, ([im.astype(np.int8)],), {}),
                          (TypeError, (px, tab), {"out": np.zeros((2, 2, 4, 3), F32)}),
                          (TypeError, (px, tab), {"out": torch.zeros((2, 2, 4, 3), dtype=torch.float64)}),
                          (ValueError, (torch.zeros(30, dtype=torch.uint8), tab), {}),                   # a host tensor
                          (ValueError, (px.reshape(2, 15), tab), {}), (ValueError, (px,), {}), (ValueError, ([im], tab), {}),
                          (ValueError, (px, [0, 2, 3, 0]), {}), (ValueError, (px, [[0, 2, 3]]), {}), (ValueError, (px, np.zeros((0, 4), np.int32)), {}),
                          (ValueError, (px, np.zeros((ops.IMAGE_MAX_FRAMES + 1, 4), np.int32)), {}),
                          (ValueError, (px, [[0, 0, 3, 0]]), {}), (ValueError, (px, [[0, 2, 0, 0]]), {}), (ValueError, (px, [[-1, 2, 3, 0]]), {}),
                          (ValueError, (px, [[13, 2, 3, 0]]), {}), (ValueError, (px, [[0, 2, 6, 0]]), {}),  # 31 and 36 bytes of 30
                          (ValueError, (px, [[2 ** 31, 1, 1, 0]]), {}),
                          (ValueError, (px, tab), {"canvas": (1, 4)}), (ValueError, (px, tab), {"canvas": (2, 3)}),      # a frame larger than the canvas
                          (ValueError, (px, tab), {"canvas": (0, 4)}), (ValueError, (px, tab), {"canvas": (2, 4, 3)}),
                          (ValueError, (px, tab), {"canvas": (2 ** 15, 2 ** 15)}),
                          (ValueError, (px, torch.zeros((2, 4), dtype=torch.int32)), {}),                # a device table: canvas=None cannot be read
                          (ValueError, (px, torch.zeros((2, 4), dtype=torch.int32)), {"canvas": (2, 4), "flip": [0, 1]}),
                          (ValueError, (px, torch.zeros((2, 4), dtype=torch.int32)), {"canvas": (2, 4)}),  # ... and it is a host tensor
                          (ValueError, (px, tab), {"flip": [1]}), (ValueError, (px, tab), {"means": [1.0, 2.0]}),
                          (ValueError, (px, tab), {"out": torch.zeros((2, 2, 4, 3))}),                   # a host tensor
                          (ValueError, ([im, im],), {"canvas": (1, 3)})):
        with pytest.raises(exc, match="image_blob|pack_image_frames"):
            ops.image_blob(*args, **kw)
    L, lib = ops.lib(), ops._lib
    A = 4096                                                                         # a non-NULL, aligned "pointer" (never dereferenced)
    m = (C.c_double * 3)(1.0, 2.0, 3.0)
    for args in ((A, 30, A, -1, m, 2, 4, A), (A, 30, A, ops.IMAGE_MAX_FRAMES + 1, m, 2, 4, A), (A, -1, A, 1, m, 2, 4, A),
                 (A, 30, A, 1, m, 0, 4, A), (A, 30, A, 1, m, 2, 0, A), (A, 30, A, 1, m, 2 ** 15, 2 ** 15, A),      # 3 * 2^30 elements
                 (A, 30, A, 1, m, 26755, 26755, A),                                  # 3 * 26755^2 = 2^31 + 6 427 elements
                 (None, 30, A, 1, m, 2, 4, A), (A, 30, None, 1, m, 2, 4, A), (A, 30, A, 1, None, 2, 4, A), (A, 30, A, 1, m, 2, 4, None),
                 (A, 30, A + 2, 1, m, 2, 4, A), (A, 30, A, 1, m, 2, 4, A + 2), (A, 30, A, 1, m, 2, 4, A + 1)):
        assert L.mv3d_image_blob(*args, None) == lib.ERR_INVALID_ARG, args
    assert L.mv3d_image_blob(None, 0, None, 0, None, 2, 4, None, None) == lib.OK      # no frame: nothing to do


def test_get_minibatch_refuses_other_images_with_the_key_on():
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch
    cfg.IMAGE_BLOB_ON_DEVICE = True
    try:
        for image in (_entry()["image"].astype(F32), _entry()["image"][:, :, 0], _entry()["image"].tolist()):
            with pytest.raises(TypeError, match="IMAGE_BLOB_ON_DEVICE"):
                get_minibatch([_entry(image=image)], 2)
    finally:
        cfg.IMAGE_BLOB_ON_DEVICE = False


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_every_value(gpu):
    """all 256 byte values in every channel under cfg.PIXEL_MEANS: a kernel that subtracts in f32 differs in 303 of the 768 pairs"""
    rng = np.random.RandomState(1)
    im = np.stack([rng.permutation(256).astype(np.uint8).reshape(16, 16) for _ in range(3)], -1)
    assert all(len(np.unique(im[:, :, c])) == 256 for c in range(3))
    got, want = device_blob(gpu, [im])
    assert got.shape == (1, 16, 16, 3) and np.array_equal(bits(got), bits(want))
    got, want = device_blob(gpu, [im], means=[0.1, 127.3, 254.9])
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.gpu
@pytest.mark.parametrize("canvas", [None, (5, 11)])
def test_every_alignment(gpu, canvas):
    """27 frames, widths 1 .. 9 and heights 1 .. 3: every residue of 3 w mod 4, odd byte offsets between frames, canvas rows of 108
    and 132 bytes whose 16-byte split moves from row to row"""
    shapes = [(h, w) for w in range(1, 10) for h in (1, 2, 3)]
    ims = images(2, shapes)
    offsets = gpu["ops"].pack_image_frames(ims)[1][:, 0]
    assert set(int(o) % 4 for o in offsets) == {0, 1, 2, 3} and set(3 * w % 4 for _, w in shapes) == {0, 1, 2, 3}
    got, want = device_blob(gpu, ims, canvas)
    assert got.shape == (27,) + (canvas or (3, 9)) + (3,) and np.array_equal(bits(got), bits(want))


@pytest.mark.gpu
def test_flip(gpu):
    torch, ops = gpu["torch"], gpu["ops"]
    ims = images(3, [(2, 1), (3, 2), (2, 5), (3, 8), (1, 8), (3, 5), (2, 2), (3, 1)])
    flip = [1, 1, 1, 1, 0, 0, 1, 0]
    got, want = device_blob(gpu, ims, flip=flip)
    assert np.array_equal(bits(got), bits(want)) and not np.array_equal(bits(got), bits(R.blob(ims)))
    got, want = device_blob(gpu, ims, (4, 9), flip=flip)
    assert np.array_equal(bits(got), bits(want))
    # a frame that fills its canvas: the flag is ops.mirror_columns of the unflipped result
    full = images(4, [(4, 7)])
    plain = ops.image_blob(full, out=nan_frames(torch, (1, 4, 7, 3)))
    flipped = ops.image_blob(full, flip=[True], out=nan_frames(torch, (1, 4, 7, 3)))
    assert torch.equal(flipped.view(torch.int32), ops.mirror_columns(plain.clone()).view(torch.int32))
    assert not torch.equal(flipped.view(torch.int32), plain.view(torch.int32))


@pytest.mark.gpu
def test_out_slice(gpu):
    """frames 1:3 of a 4-frame buffer of (3, 5, 3) frames: 180 bytes a frame, so the slice starts 4 mod 16"""
    torch, ops = gpu["torch"], gpu["ops"]
    ims = images(5, [(3, 5), (2, 4)])
    big = nan_frames(torch, (4, 3, 5, 3))
    out = big[1:3]
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    assert ops.image_blob(ims, canvas=(3, 5), out=out) is out
    host = big.cpu().numpy()
    assert np.array_equal(bits(host[1:3]), bits(R.blob(ims, (3, 5))))
    nan = bits(np.full((3, 5, 3), np.nan, F32))
    assert np.array_equal(bits(host[0]), nan) and np.array_equal(bits(host[3]), nan)


@pytest.mark.gpu
def test_malformed_device_table(gpu):
    """rows the kernel must not use, between well-formed neighbours.  `pixels` is a window into a longer buffer and `out` a run of
    frames with a guard frame on each side, so a kernel that ignored a check would still stay inside this test's allocations and show
    up as a wrong value"""
    torch, ops = gpu["torch"], gpu["ops"]
    Hc, Wc, T, lead = 4, 6, 200, 5
    rng = np.random.RandomState(6)
    store = rng.randint(1, 256, lead + T + 64).astype(np.uint8)
    window = store[lead:lead + T]                                                     # pixels[0 : total_bytes]; bytes before and behind it exist
    table = np.array([[0, 3, 5, 0],                                                   # well-formed
                      [45, Hc + 1, 2, 0], [45, 1, Wc + 1, 0], [45, 0, 3, 0], [45, 3, 0, 1], [-1, 1, 1, 0],
                      [T + 1 - 3 * 2 * 3, 2, 3, 0],                                  # offset + size = total_bytes + 1
                      [T - 3 * 4 * 6, 4, 6, 1],                                       # well-formed: ends exactly at total_bytes, fills its canvas
                      [101, 2, 3, 1]], np.int32)                     # well-formed, odd offset
    good = [0, 7, 8]
    big = nan_frames(torch, (len(table) + 2, Hc, Wc, 3))
    d_store = torch.from_numpy(store).cuda()
    got = ops.image_blob(d_store[lead:lead + T], torch.from_numpy(table).cuda(), canvas=(Hc, Wc), out=big[1:-1])
    host = big.cpu().numpy()
    nan = bits(np.full((Hc, Wc, 3), np.nan, F32))
    assert np.array_equal(bits(host[0]), nan) and np.array_equal(bits(host[-1]), nan)
    assert got.data_ptr() == big[1:-1].data_ptr()
    for b, (o, h, w, f) in enumerate(table):
        if b in good:
            want = R.blob([window[o:o + 3 * h * w].reshape(h, w, 3)], (Hc, Wc), flip=[f])[0]
            assert want.any()
        else:
            want = np.zeros((Hc, Wc, 3), F32)
        assert np.array_equal(bits(host[1 + b]), bits(want)), (b, table[b])


@pytest.mark.gpu
def test_workload_shape(gpu):
    """two KITTI sizes on the (376, 1242) canvas: the grid and the index arithmetic at full row length (5.6 MB written)"""
    ims = images(7, [(376, 1241), (370, 1224)])
    got, want = device_blob(gpu, ims, (376, 1242), flip=[0, 1])
    assert got.shape == (2, 376, 1242, 3) and np.array_equal(bits(got), bits(want))


@pytest.mark.gpu
def test_capture_and_replay(gpu):
    torch, ops = gpu["torch"], gpu["ops"]
    cap, canvas = 3 * 5 * 9 * 2 + 7, (5, 9)
    fillings = []
    for seed, shapes, flip in ((10, [(5, 9), (2, 3)], [0, 1]), (11, [(1, 7), (4, 8)], [1, 0])):
        ims = images(seed, shapes)
        px, tab, _ = ops.pack_image_frames(ims)
        tab[:, 3] = flip
        buf = np.random.RandomState(seed).randint(0, 256, cap).astype(np.uint8)      # the whole buffer is refilled: stale bytes behind the frames
        buf[:len(px)] = px
        fillings.append((buf, tab, R.blob(ims, canvas, flip=flip)))
    d_px = torch.from_numpy(fillings[0][0]).cuda()
    d_tab = torch.from_numpy(fillings[0][1]).cuda()
    big = nan_frames(torch, (4,) + canvas + (3,))
    out = big[1:3]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.image_blob(d_px, d_tab, canvas=canvas, out=out)                           # (warm-up: the code object is loaded outside the capture)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.image_blob(d_px, d_tab, canvas=canvas, out=out)
    nan = bits(np.full(canvas + (3,), np.nan, F32))
    for buf, tab, want in reversed(fillings):
        d_px.copy_(torch.from_numpy(buf))
        d_tab.copy_(torch.from_numpy(tab))
        big.fill_(float("nan"))
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        host = big.cpu().numpy()
        assert np.array_equal(bits(host[1:3]), bits(want))
        assert np.array_equal(bits(host[0]), nan) and np.array_equal(bits(host[3]), nan)


@pytest.mark.gpu
def test_get_minibatch_builds_the_blob_on_the_device(gpu):
    torch = gpu["torch"]
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.roi_data_layer.minibatch_mv3d import get_minibatch

    def host(t):
        return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    try:
        for flipped in (False, True):
            entry = _entry(flipped=flipped)
            cfg.IMAGE_BLOB_ON_DEVICE, cfg.IMAGE_CANVAS = False, None
            off = get_minibatch([entry], 2)
            assert isinstance(off["image_data"], torch.Tensor) == flipped            # (a mirrored frame's maps are device tensors already)
            cfg.IMAGE_BLOB_ON_DEVICE = True
            on = get_minibatch([entry], 2)
            img = on["image_data"]
            assert isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.float32 and tuple(img.shape) == (1, 8, 12, 3)
            assert np.array_equal(bits(host(img)), bits(host(off["image_data"])))
            assert np.array_equal(bits(host(img)), bits(R.blob([entry["image"]], flip=[flipped])))
            assert set(on) == set(off) and np.array_equal(bits(host(on["lidar_bv_data"])), bits(host(off["lidar_bv_data"])))
            cfg.IMAGE_CANVAS = (9, 14)
            padded = get_minibatch([entry], 2)
            assert tuple(padded["image_data"].shape) == (1, 9, 14, 3)
            assert np.array_equal(bits(host(padded["image_data"])), bits(R.blob([entry["image"]], (9, 14), flip=[flipped])))
            for k in ("im_info", "calib", "gt_boxes", "gt_boxes_bv", "gt_boxes_3d", "gt_boxes_corners"):
                assert np.array_equal(padded[k], off[k]) and np.array_equal(on[k], off[k]), k
            cfg.IMAGE_CANVAS = (8, 11)
            with pytest.raises(ValueError, match="larger than the canvas"):
                get_minibatch([entry], 2)
    finally:
        cfg.IMAGE_BLOB_ON_DEVICE, cfg.IMAGE_CANVAS = False, None


@pytest.mark.gpu
def test_detection_loops_pad_the_images(gpu, tmp_path):
    torch, ops = gpu["torch"], gpu["ops"]
    from mv3d_tf_amd.fast_rcnn import detect_batch
    from mv3d_tf_amd.fast_rcnn.config import cfg
    from mv3d_tf_amd.rpn_msr.generate import imdb_proposals
    rois = np.array([[0, 20, 1, -1, 4, 1.6, 1.5], [0, 30, -3, -1, 4, 1.6, 1.5]], F32)
    bev = np.random.RandomState(12).random_sample((16, 16, 9)).astype(F32)

    def host(t):
        return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)

    class Net:
        """a stub that records the images it is fed and answers with two fixed ROIs per frame whose scores depend on the frame's image"""
        views = 2

        def __init__(self):
            self.fed, self.on_device = [], []

        def forward(self, feed):
            self.on_device.append(isinstance(feed["image_data"], torch.Tensor) and feed["image_data"].is_cuda)
            img = host(feed["image_data"])
            self.fed.append(img)
            B = img.shape[0]
            assert img.dtype == F32 and host(feed["lidar_bv_data"]).shape == (B, 16, 16, 9) and np.array_equal(feed["im_info"], [[16, 16, 1]] * B)
            p = np.array([0.3 + 0.4 * ((float(img[b].sum(dtype=np.float64)) * 0.37) % 1.0) for b in range(B)], F32)
            scores = np.stack([np.stack([1 - p, p], 1), np.stack([p, 1 - p], 1)], 1).reshape(2 * B, 2)
            r3, r4 = np.tile(rois, (B, 1)), np.tile(rois[:, :5], (B, 1))
            r3[:, 0] = r4[:, 0] = np.repeat(np.arange(B), 2)
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            return {"rois": (dev(r4), dev(r4 + 1), dev(r3)), "cls_prob": dev(scores), "bbox_pred": dev(np.zeros((2 * B, 48), F32)),
                    "num_rois": dev(np.full((B,), 2, np.int32)), "rois_per_frame": 2, "rois_status": dev(np.zeros((B,), np.int32))}

    class Imdb:
        name, num_classes, image_index = "four_images", 2, ["000000", "000001", "000002", "000003"]

        def __init__(self, ims): self.ims = ims
        def image_at(self, i): return self.ims[i]
        def bv_at(self, i): return bev
        def calib_at(self, i): return np.zeros((4, 12))
        def evaluate_detections(self, *a): self.evaluated = True

    mixed = images(13, [(8, 12), (8, 12), (7, 11), (8, 13)])
    equal = images(14, [(8, 12)] * 4)

    def run(loop, ims):
        net = Net()
        res = detect_batch.test_net(None, net, Imdb(ims), "w") if loop == "test_net" else imdb_proposals(None, net, Imdb(ims))
        return net, res

    saved, root = dict(cfg.TEST), cfg.ROOT_DIR
    cfg.ROOT_DIR = str(tmp_path)
    try:
        cfg.TEST.BATCH_SIZE = 4
        for loop in ("test_net", "imdb_proposals"):
            cfg.IMAGE_BLOB_ON_DEVICE, cfg.IMAGE_CANVAS = False, None
            net, _ = run(loop, mixed)                                                 # key off: a group ends at every change of image shape
            assert [f.shape for f in net.fed] == [(2, 8, 12, 3), (1, 7, 11, 3), (1, 8, 13, 3)] and not any(net.on_device)
            for fed, g in zip(net.fed, ([0, 1], [2], [3])):
                assert np.array_equal(bits(fed), bits(R.blob([mixed[i] for i in g])))
            _, off = run(loop, equal)
            cfg.IMAGE_BLOB_ON_DEVICE = True
            net, on = run(loop, equal)                                                # equal shapes: the same blob, the same results
            assert net.on_device == [True] and np.array_equal(bits(net.fed[0]), bits(R.blob(equal)))
            if loop == "test_net":
                for a, b in zip(on, off):                                             # (all_boxes, all_boxes_cnr)[class][frame]
                    assert all(len(a[1][i]) >= 1 and np.array_equal(a[1][i], b[1][i]) for i in range(4))
                assert not np.array_equal(off[0][1][0][:, -1], off[0][1][1][:, -1])   # the scores do depend on the image
            else:
                assert all(np.array_equal(on[k][i], off[k][i]) and len(on[k][i]) == 2 for k in ("bv", "image") for i in range(4))
            net, _ = run(loop, mixed)                                                 # key on: ONE forward, the group's maximal shape
            assert net.on_device == [True] and net.fed[0].shape == (4, 8, 13, 3)
            assert np.array_equal(bits(net.fed[0]), bits(R.blob(mixed)))
            cfg.IMAGE_CANVAS = (9, 16)
            net, _ = run(loop, mixed)
            assert net.on_device == [True] and net.fed[0].shape == (4, 9, 16, 3)
            assert np.array_equal(bits(net.fed[0]), bits(R.blob(mixed, (9, 16))))
            cfg.IMAGE_CANVAS = (7, 16)
            net = Net()
            with pytest.raises(ValueError, match="larger than the canvas"):
                detect_batch.test_net(None, net, Imdb(mixed), "w") if loop == "test_net" else imdb_proposals(None, net, Imdb(mixed))
            assert net.fed == []                                                      # refused before any forward
        cfg.IMAGE_CANVAS = None
        cfg.TEST.BATCH_SIZE = 1                                                       # the key alone selects the device route
        net, _ = run("test_net", equal)
        assert net.on_device == [True] * 4 and all(f.shape == (1, 8, 12, 3) for f in net.fed)
        # image_feed(out=): the canvas is the buffer's, the way into a captured graph's static input
        static = nan_frames(torch, (4, 9, 14, 3))
        assert detect_batch.image_feed(mixed, out=static) is static
        assert np.array_equal(bits(static.cpu().numpy()), bits(R.blob(mixed, (9, 14))))
    finally:
        cfg.IMAGE_BLOB_ON_DEVICE, cfg.IMAGE_CANVAS = False, None
        cfg.TEST.clear()
        cfg.TEST.update(saved)
        cfg.ROOT_DIR = root

"""What the detection loops (fast_rcnn.test_mv.test_net, fast_rcnn.detect_batch.test_net, rpn_msr.generate.imdb_proposals) share in
front of the network: the image read, the frame loader and the lazy group iterator.  No device."""
import numpy as np
import pytest


def test_load_frame_from_arrays_and_from_files(tmp_path):
    from mv3d_tf_amd.fast_rcnn.loop_parts import load_frame
    rng = np.random.RandomState(3)
    im = rng.randint(0, 255, (3, 4, 3)).astype(np.uint8)
    bv = rng.random_sample((5, 6, 9)).astype(np.float32)
    calib = rng.random_sample((4, 12))
    np.save(str(tmp_path / "im.npy"), im)
    np.save(str(tmp_path / "bv.npy"), bv)

    class Arrays:
        def image_at(self, i): return im
        def bv_at(self, i): return bv
        def calib_at(self, i): return calib

    class Paths:
        def image_path_at(self, i): return str(tmp_path / "im.npy")
        def lidar_path_at(self, i): return str(tmp_path / "bv.npy")
        def calib_at(self, i): return calib

    for got in (load_frame(Arrays(), 0), load_frame(Paths(), 0)):
        assert len(got) == 3 and np.array_equal(got[0], im) and np.array_equal(got[1], bv) and np.array_equal(got[2], calib)
        assert got[0].dtype == np.uint8 and got[1].dtype == np.float32

    def refuse(self, i):
        raise AssertionError("stored_bv=False must not open the stored map")

    for base in (Arrays, Paths):                             # stored_bv=False: neither source of the stored map is touched
        imdb = type("NoMap", (base,), dict(bv_at=refuse, lidar_path_at=refuse))()
        got = load_frame(imdb, 0, stored_bv=False)
        assert np.array_equal(got[0], im) and got[1] is None and np.array_equal(got[2], calib)
        with pytest.raises(AssertionError):
            load_frame(imdb, 0)


def test_read_image_bgr(tmp_path):
    from mv3d_tf_amd.utils.read_image import read_image_bgr
    im = np.random.RandomState(4).randint(0, 255, (3, 4, 3)).astype(np.uint8)
    np.save(str(tmp_path / "im.npy"), im)
    got = read_image_bgr(str(tmp_path / "im.npy"))
    assert got.dtype == np.uint8 and np.array_equal(got, im)
    Image = pytest.importorskip("PIL.Image")
    Image.fromarray(im, "RGB").save(str(tmp_path / "im.png"))
    got = read_image_bgr(str(tmp_path / "im.png"))
    assert got.dtype == np.uint8 and np.array_equal(got, im[:, :, ::-1])


def test_every_reader_is_the_one_reader():
    from mv3d_tf_amd.fast_rcnn import loop_parts, test_mv
    from mv3d_tf_amd.roi_data_layer import minibatch_mv3d
    from mv3d_tf_amd.utils.read_image import read_image_bgr
    assert minibatch_mv3d.read_image_bgr is read_image_bgr and loop_parts.read_image_bgr is read_image_bgr
    assert test_mv.load_frame is loop_parts.load_frame


def test_groups_load_their_frames_lazily():
    from mv3d_tf_amd.fast_rcnn.detect_batch import iter_loaded_groups
    a, b = np.zeros((8, 12, 3), np.uint8), np.zeros((7, 11, 3), np.uint8)
    bv = np.zeros((16, 16, 9), np.float32)

    class Imdb:
        image_index = ["0", "1", "2", "3", "4"]
        loaded = []

        def image_at(self, i):
            self.loaded.append(i)
            return [a, a, b, a, a][i]

        def bv_at(self, i): return bv
        def calib_at(self, i): return i

    imdb = Imdb()
    it = iter_loaded_groups(imdb, None, False, 2)
    group, (ims, bvs, calibs, clouds) = next(it)
    assert group == [0, 1] and len(imdb.loaded) <= 3         # the frame that ended the group, and none behind it
    assert all(x is a for x in ims) and all(x is bv for x in bvs) and len(ims) == len(bvs) == 2
    assert calibs == (0, 1) and clouds == (None, None)
    rest = list(it)
    assert [g for g, _ in rest] == [[2], [3, 4]] and imdb.loaded == [0, 1, 2, 3, 4]
    assert rest[0][1][0][0] is b and rest[1][1][2] == (3, 4)

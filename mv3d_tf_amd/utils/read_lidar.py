"""`point_cloud_2_top`: interface of lib/utils/read_lidar.py:10-115 (== tools/read_lidar.py), every parameter of it.

The call MV3D makes (tools/read_lidar.py:121-133: res=0.1, zres=0.3, side_range=(-30,30), fwd_range=(0,60), height_range=(-2,0.4) ->
(601,601,9)) goes through mv3d_point_cloud_2_top, any other parameter set through mv3d_point_cloud_2_top_ranges (which reports the
cells numpy would refuse: IndexError here as there).

`point_cloud_2_top_paper`: the same points -> the MV3D paper's encoding of the bird's-eye view (not in the reference).
`point_cloud_2_front`: the same points -> the (64,512,3) front-view map [height, distance, intensity] of the third view (not in the
reference; ops.point_cloud_2_front).  `load_velodyne`: a KITTI `velodyne/*.bin` scan (or a `.npy`) as (P,4) f32."""
import numpy as np
import torch

from .. import ops

_MV3D = (0.1, 0.3, -30., 30., 0., 60., -2., 0.4)


def point_cloud_2_top(points, res=0.1, zres=0.3, side_range=(-10., 10.), fwd_range=(-10., 10.), height_range=(-2., 2.)):
    """defaults as lib/utils/read_lidar.py:10-16"""
    got = (float(res), float(zres), float(side_range[0]), float(side_range[1]), float(fwd_range[0]), float(fwd_range[1]),
           float(height_range[0]), float(height_range[1]))
    as_numpy = not isinstance(points, torch.Tensor)
    pts = ops._dev(np.ascontiguousarray(points, dtype=np.float32)[:, :4] if as_numpy else points[:, :4])
    top = ops.point_cloud_2_top(pts, None if got == _MV3D else got)
    return top.cpu().numpy() if as_numpy else top


def point_cloud_2_top_paper(points, res=0.1, zres=0.3, side_range=(-30., 30.), fwd_range=(0., 60.), height_range=(-2., 0.4)):
    """(P,4+) [x,y,z,reflectance] -> the MV3D paper's BEV encoding (ops.point_cloud_2_top_paper, DESIGN.md section 3.24: slice maxima,
    the highest point's reflectance, density); the defaults are the call MV3D makes -> (601,601,10).  numpy in, numpy out (a device
    tensor in, a device tensor out); IndexError where point_cloud_2_top raises it."""
    got = (float(res), float(zres), float(side_range[0]), float(side_range[1]), float(fwd_range[0]), float(fwd_range[1]),
           float(height_range[0]), float(height_range[1]))
    as_numpy = not isinstance(points, torch.Tensor)
    top = ops.point_cloud_2_top_paper(np.ascontiguousarray(points, dtype=np.float32)[:, :4] if as_numpy else points[:, :4].contiguous(),
                                      ranges=None if got == _MV3D else got)
    return top.cpu().numpy() if as_numpy else top


def point_cloud_2_front(points):
    """(P,4+) [x,y,z,reflectance] -> (64,512,3) f32 front-view map; numpy in, numpy out (a device tensor in, a device tensor out)"""
    as_numpy = not isinstance(points, torch.Tensor)
    fv = ops.point_cloud_2_front(np.ascontiguousarray(points, dtype=np.float32)[:, :4] if as_numpy else points[:, :4])
    return fv.cpu().numpy() if as_numpy else fv


def load_velodyne(path):
    """A Velodyne scan file -> (P,4) f32 [x,y,z,reflectance]: KITTI's raw little-endian f32 quadruples (`.bin`), or a `.npy` array"""
    if path.endswith(".npy"):
        return np.ascontiguousarray(np.load(path), dtype=np.float32).reshape(-1, 4)
    return np.fromfile(path, dtype=np.float32).reshape(-1, 4)

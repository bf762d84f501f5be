// Left/right mirror of a training frame's maps, in place: a contiguous (rows, width, channels) f32 array gets
// data[r][w][c] <- data[r][width - 1 - w][c].  One thread per element PAIR (w, width - 1 - w), w < width / 2: it reads both
// elements and writes both, so every element is read once and written once, there is no workspace, and no two threads touch the
// same address (the middle column of an odd width belongs to no pair).  blockIdx.x / threadIdx.x run over the width / 2 * channels
// floats of a row's left half, which are contiguous, so a wave's loads and stores on the left are coalesced; its partners on the
// right are the same pixels in descending order, `channels` consecutive floats each, and fall into the same cache lines as a
// forward sweep would.  Pixels are 12 and 36 bytes in the two maps of a frame, so nothing here assumes vector alignment: plain
// dword accesses.  Rows go over blockIdx.y with a stride, offsets are 64-bit.
#include "common.h"

#define MIRROR_BLOCK 256

__global__ __launch_bounds__(MIRROR_BLOCK) void mirror_columns_kernel(float *__restrict__ data, long long rows, int width, int channels,
                                                                      unsigned left)     // left = width / 2 * channels
{
    const unsigned q = blockIdx.x * MIRROR_BLOCK + threadIdx.x;                          // float q of the row's left half
    if (q >= left) return;
    const unsigned p = q / (unsigned)channels, c = q - p * (unsigned)channels;           // pixel and channel
    const long long row_elems = (long long)width * channels;
    const long long mirrored = (long long)(width - 1 - (int)p) * channels + c;
    for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
        float *row = data + r * row_elems;
        const float a = row[q], b = row[mirrored];
        row[q] = b;
        row[mirrored] = a;
    }
}

extern "C" int mv3d_mirror_columns(float *data_dev, long long rows, int width, int channels, void *stream)
{
    if (rows < 0 || width < 1 || channels < 1) return MV3D_ERR_INVALID_ARG;
    if ((long long)width * channels > 0x7fffffffLL) return MV3D_ERR_INVALID_ARG;         // a row is indexed with 32 bits
    if (rows > 0 && !data_dev) return MV3D_ERR_INVALID_ARG;
    const unsigned left = (unsigned)(width / 2) * (unsigned)channels;
    if (rows == 0 || left == 0) return MV3D_OK;
    const dim3 grid((left + MIRROR_BLOCK - 1) / MIRROR_BLOCK, (unsigned)(rows < 65535 ? rows : 65535));
    hipLaunchKernelGGL(mirror_columns_kernel, grid, dim3(MIRROR_BLOCK), 0, (hipStream_t)stream, data_dev, rows, width, channels, left);
    return mv3d_launch_status();
}

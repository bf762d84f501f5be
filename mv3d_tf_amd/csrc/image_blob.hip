// Image input: `num_frames` uint8 BGR frames of their own sizes, back to back in one byte buffer -> the
// (num_frames, canvas_h, canvas_w, 3) f32 blob the image trunk reads, in ONE launch.  Frame b lies at the top-left corner of its
// canvas (lib/utils/blob.py:14-27, im_list_to_blob), everything else of the canvas is +0.0f:
//   out[b][y][x][c] = (float)((double)src_b[y][x'][c] - means[c])   for y < h_b, x < w_b;  x' = flip_b ? w_b - 1 - x : x
// -- the host expression (np.asarray(im, np.float64) - PIXEL_MEANS).astype(np.float32), ONE rounding from f64.  A byte has 256 values,
// so every workgroup computes the 3 x 256 results once, in f64, into LDS (3 KB), and an element is one byte load and one lookup.
//   rows     a workgroup works on ONE canvas row (b, y), a run of canvas_w * 3 floats: an output float q of the row is channel q % 3
//            of pixel q / 3 (a division by a constant), and of an unflipped frame it is source byte q of the frame's row y.  The
//            frame (b = row / canvas_h, one division per workgroup) and its table row are the same for all of its threads.
//   stores   a canvas row is canvas_w * 12 bytes (14 904 = 8 mod 16 at 1242 columns) and out_dev is only 4-byte aligned, so every row
//            has its own split: `head` scalar floats up to the row's first 16-byte boundary, 16-byte vectors (a wave stores 1 KB
//            contiguous per instruction), `tail` scalar floats -- at most 3 + 3 scalar stores in a row, by the row's first workgroup.
//            Every element of out is written exactly once, padding included; there is no clear in front.
//   loads    bytes, at the frame's own byte alignment (a row is 3 * w_b bytes): four single-byte loads per vector, consecutive
//            lanes on consecutive bytes; a flipped frame reads the same bytes, pixels descending.
//   frames   the table is read on the device.  A row [offset, h, w, flip] is USED only if offset >= 0, 1 <= h <= canvas_h,
//            1 <= w <= canvas_w and offset + 3 h w <= total_bytes (64-bit); otherwise the frame's canvas is all zeros.  A byte is
//            read at offset + 3 w y + s with y < h and s < 3 w, below offset + 3 h w, and a store goes to the row the workgroup
//            owns: no value in the table can make the call read outside pixels_dev[0 : total_bytes] or write outside out.
// Bound by the f32 stores (12 B written per 3 B read).
#include "common.h"

#define IMB_BLOCK 256
#define IMB_VECS 4                                      // 16-byte vectors per thread: a workgroup covers 1024 vectors = 16 KB of a row

// Source byte of float q of a row that HAS pixels (row_bytes = 3 * w_b >= 3): channel q % 3 of pixel q / 3, read from the mirrored
// pixel of a flipped frame.  Behind the frame's last column the index is clamped to byte 0 of the row, so that every load of a
// thread is unconditional and all of them are in flight together; imb_pick then drops what was read.
__device__ __forceinline__ int imb_source(int q, int row_bytes, bool flip, int &c)
{
    const int qq = q < row_bytes ? q : 0;
    const int x = qq / 3;
    c = qq - 3 * x;
    return flip ? row_bytes - 3 - 3 * x + c : qq;        // (w - 1 - x) * 3 + c
}

__device__ __forceinline__ float imb_pick(const float *s_tab, int q, int row_bytes, int c, unsigned byte)
{
    const float t = s_tab[c * 256 + (int)byte];
    return q < row_bytes ? t : 0.0f;
}

// One canvas row.  PIXELS: the frame has this row (row_bytes >= 3, src_row its first byte); otherwise the row is padding or the
// frame's table row is not used, and zeros are stored without a load.
template <bool PIXELS>
__device__ __forceinline__ void imb_row(const uint8_t *__restrict__ src_row, const float *s_tab, int row_bytes, bool flip,
                                        float *__restrict__ dst, int head, int nvec, int tail, int chunk)
{
    const int v0 = chunk * (IMB_BLOCK * IMB_VECS) + (int)threadIdx.x;
    unsigned byte[IMB_VECS][4];
    int c[IMB_VECS][4];
    if (PIXELS) {
#pragma unroll
        for (int u = 0; u < IMB_VECS; ++u) {
            const int v = v0 + u * IMB_BLOCK;
            const int q = head + 4 * (v < nvec ? v : 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) byte[u][j] = src_row[imb_source(q + j, row_bytes, flip, c[u][j])];
        }
    }
#pragma unroll
    for (int u = 0; u < IMB_VECS; ++u) {
        const int v = v0 + u * IMB_BLOCK;
        if (v >= nvec) continue;
        const int q = head + 4 * v;
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (PIXELS) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = imb_pick(s_tab, q + j, row_bytes, c[u][j], byte[u][j]);
        }
        *reinterpret_cast<float4 *>(dst + q) = make_float4(o[0], o[1], o[2], o[3]);
    }
    if (chunk == 0 && (int)threadIdx.x < head + tail) {
        const int q = (int)threadIdx.x < head ? (int)threadIdx.x : 4 * nvec + (int)threadIdx.x;      // (head + 4 nvec + (t - head))
        float o = 0.0f;
        if (PIXELS) {
            int cq;
            const unsigned bq = src_row[imb_source(q, row_bytes, flip, cq)];
            o = imb_pick(s_tab, q, row_bytes, cq, bq);
        }
        dst[q] = o;
    }
}

__global__ __launch_bounds__(IMB_BLOCK) void image_blob_kernel(const uint8_t *__restrict__ pixels, long long total_bytes,
                                                               const int32_t *__restrict__ frames, double m0, double m1, double m2,
                                                               int canvas_h, int row_elems, int chunks, float *__restrict__ out)
{
    __shared__ float s_tab[3 * 256];
    {
        const double v = (double)threadIdx.x;            // (IMB_BLOCK == 256: thread t owns byte value t)
        s_tab[threadIdx.x] = (float)(v - m0);
        s_tab[256 + threadIdx.x] = (float)(v - m1);
        s_tab[512 + threadIdx.x] = (float)(v - m2);
    }
    const long long row = blockIdx.x / (unsigned)chunks; // (b, y) flat
    const int chunk = (int)(blockIdx.x - (unsigned)(row * chunks));
    const int b = (int)(row / canvas_h), y = (int)(row - (long long)b * canvas_h);
    const int off = frames[4 * b], h = frames[4 * b + 1], w = frames[4 * b + 2];
    const bool flip = frames[4 * b + 3] != 0;
    const bool used = off >= 0 && h >= 1 && w >= 1 && h <= canvas_h && 3LL * w <= (long long)row_elems &&
                      (long long)off + 3LL * h * w <= total_bytes;
    float *dst = out + row * row_elems;
    const int to_boundary = (int)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) / 4u);      // 0 .. 3 floats
    const int head = to_boundary < row_elems ? to_boundary : row_elems;
    const int nvec = (row_elems - head) / 4, tail = row_elems - head - 4 * nvec;
    __syncthreads();
    if (used && y < h)                                   // (the same for every thread of the workgroup)
        imb_row<true>(pixels + ((long long)off + (long long)y * (3 * w)), s_tab, 3 * w, flip, dst, head, nvec, tail, chunk);
    else
        imb_row<false>(nullptr, s_tab, 0, false, dst, head, nvec, tail, chunk);
}

extern "C" int mv3d_image_blob(const uint8_t *pixels_dev, int total_bytes, const int32_t *frames_dev, int num_frames,
                               const double *means3_host, int canvas_h, int canvas_w, float *out_dev, void *stream)
{
    if (num_frames < 0 || num_frames > MV3D_IMAGE_MAX_FRAMES || total_bytes < 0 || canvas_h < 1 || canvas_w < 1) return MV3D_ERR_INVALID_ARG;
    if ((long long)canvas_h * canvas_w * 3 > 0x7fffffffLL) return MV3D_ERR_INVALID_ARG;       // a canvas is indexed with 32 bits
    if (num_frames == 0) return MV3D_OK;
    if (!frames_dev || !means3_host || !out_dev || (total_bytes > 0 && !pixels_dev)) return MV3D_ERR_INVALID_ARG;
    if (((uintptr_t)frames_dev & 3) != 0 || ((uintptr_t)out_dev & 3) != 0) return MV3D_ERR_INVALID_ARG;
    const int row_elems = canvas_w * 3;
    const int per_group = IMB_BLOCK * IMB_VECS;
    const int chunks = (row_elems / 4 + per_group - 1) / per_group > 0 ? (row_elems / 4 + per_group - 1) / per_group : 1;
    const long long groups = (long long)num_frames * canvas_h * chunks;
    if (groups > 0x7fffffffLL) return MV3D_ERR_INVALID_ARG;
    hipLaunchKernelGGL(image_blob_kernel, dim3((unsigned)groups), dim3(IMB_BLOCK), 0, (hipStream_t)stream, pixels_dev, (long long)total_bytes,
                       frames_dev, means3_host[0], means3_host[1], means3_host[2], canvas_h, row_elems, chunks, out_dev);
    return mv3d_launch_status();
}

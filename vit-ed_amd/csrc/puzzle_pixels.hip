// The classical Paikin-Tal baseline's pixel work on the device (solver_driver.py): an image is cut into eroded
// pieces, the pieces give the prediction-based border distances Dq int32 [4, n, n] that vited_puzzle_compat_init takes, the pieces
// are upscaled to the model's size for the learned path, and the solved board is assembled as an image.  puzzle_pixels.h states every
// per-element rule; tools/puzzle_pixels_host_check.cpp runs the same text on the host, and tests/puzzle_pixels_cases.py restates it in
// numpy.  All results are integers formed without atomics: the same bits on every call, whatever the tiling.
// Type-2 puzzles (pieces of unknown rotation) add the distances of all 16 side pairings, Dq2 int32 [4, n, n, 4],
// and a board whose pieces enter turned; tools/puzzle_type2_host_check.cpp and tests/puzzle_type2_cases.py restate those.
#include "common.h"
#include "puzzle_pixels.h"

namespace {

namespace pp = puzzle_pixels;

constexpr int PP_THREADS = 256;

// ---- cut: one thread per output pixel -----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PP_THREADS)
puzzle_cut_kernel(const uint8_t* __restrict__ image, pp::Cut g, const int* __restrict__ order, int64_t n, uint8_t* __restrict__ pieces) {
    const int64_t area = (int64_t)g.We * g.We;
    const int64_t idx = (int64_t)blockIdx.x * PP_THREADS + threadIdx.x;
    if (idx >= n * area) return;
    const int64_t k = idx / area;
    const int64_t rem = idx - k * area;
    int64_t cell = order ? order[k] : k;
    cell = cell < 0 ? 0 : (cell >= n ? n - 1 : cell);          // a device-side argument: clamped, never an index outside the image
    const uint8_t* src = image + pp::cut_source(g, cell, (int)(rem / g.We), (int)(rem % g.We));
    uint8_t* dst = pieces + idx * pp::CHANNELS;
    dst[0] = src[0], dst[1] = src[1], dst[2] = src[2];
}

// ---- resize: one workgroup per piece; the S taps (the same for rows and columns) are formed once, in LDS -------------------------------
constexpr int PP_MAX_SIZE = 1024;

__global__ void __launch_bounds__(PP_THREADS)
puzzle_resize_kernel(const uint8_t* __restrict__ pieces, int We, int S, uint8_t* __restrict__ out) {
    __shared__ pp::Taps taps[PP_MAX_SIZE];
    for (int x = threadIdx.x; x < S; x += PP_THREADS) taps[x] = pp::resample_taps(We, S, x);
    __syncthreads();
    const uint8_t* piece = pieces + (int64_t)blockIdx.x * We * We * pp::CHANNELS;
    uint8_t* o = out + (int64_t)blockIdx.x * pp::CHANNELS * S * S;
    const int plane = S * S;
    for (int idx = threadIdx.x; idx < pp::CHANNELS * plane; idx += PP_THREADS) {
        const int c = idx / plane, rem = idx - c * plane;
        o[idx] = pp::resample_pixel(piece, We, taps[rem / S], taps[rem % S], c);
    }
}

// ---- distances -------------------------------------------------------------------------------------------------------------------------
// Pass 1: the strips.  strips[0][s][i] is the prediction of side s of piece i, strips[1][s][i] its border, `padded` uint16 each.
__global__ void __launch_bounds__(PP_THREADS)
puzzle_strips_kernel(const uint8_t* __restrict__ pieces, int64_t n, int We, int padded, uint16_t* __restrict__ strips) {
    const int64_t idx = (int64_t)blockIdx.x * PP_THREADS + threadIdx.x;
    const int64_t per_kind = 4 * n * padded;
    if (idx >= 2 * per_kind) return;
    const int kind = idx >= per_kind;
    const int64_t rem = idx - kind * per_kind;
    const int k = (int)(rem % padded);
    const int64_t si = rem / padded;                            // s * n + i
    const int s = (int)(si / n);
    const uint8_t* piece = pieces + (si - s * n) * We * We * pp::CHANNELS;
    strips[idx] = kind ? pp::strip_border(piece, We, s, k) : pp::strip_prediction(piece, We, s, k);
}

// Pass 2: all pairs.  A workgroup owns the PD_TILE x PD_TILE block (i0.., j0..) of one side and walks the strips in stages of PD_STAGE
// values: the predictions of its 32 i and the facing borders of its 32 j are staged in LDS, and thread (ty, tx) accumulates the four
// outputs (i0 + ty + 8 a, j0 + tx) with v_sad_u16 on 8-byte reads.  A staged row is PD_ROW = 68 uint16 = 34 dwords long: the 32 lanes of a
// half-wave read 32 different border rows with ds_read_b64, rows 34 dwords apart start on the 32 different even banks of the 64, so the
// read is conflict-free; their prediction row is one address, a broadcast.
constexpr int PD_TILE = 32;
constexpr int PD_STAGE = 64;
constexpr int PD_ROW = PD_STAGE + 4;
constexpr int PD_PER_THREAD = PD_TILE * PD_TILE / PP_THREADS;   // 4

__global__ void __launch_bounds__(PP_THREADS)
puzzle_pixel_distances_kernel(const uint16_t* __restrict__ strips, int64_t n, int padded, int* __restrict__ dq) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[2][PD_TILE * PD_ROW];
    const int s = blockIdx.z;
    const int64_t i0 = (int64_t)blockIdx.y * PD_TILE, j0 = (int64_t)blockIdx.x * PD_TILE;
    const int tx = threadIdx.x % PD_TILE, ty = threadIdx.x / PD_TILE;
    const uint16_t* pred = strips + (int64_t)s * n * padded;
    const uint16_t* face = strips + (int64_t)(4 + ((s + 2) & 3)) * n * padded;
    uint32_t acc[PD_PER_THREAD] = {0u, 0u, 0u, 0u};
    for (int k0 = 0; k0 < padded; k0 += PD_STAGE) {
        const int items = (padded - k0 < PD_STAGE ? padded - k0 : PD_STAGE) / 4;       // 8-byte items of this stage, per row
        for (int idx = threadIdx.x; idx < 2 * PD_TILE * (PD_STAGE / 4); idx += PP_THREADS) {
            const int which = idx / (PD_TILE * (PD_STAGE / 4)), rem = idx % (PD_TILE * (PD_STAGE / 4));
            const int r = rem / (PD_STAGE / 4), q = rem % (PD_STAGE / 4);
            if (q >= items) continue;
            const int64_t piece = (which ? j0 : i0) + r;
            uint2 v = make_uint2(0u, 0u);                       // rows past n: zeros, their outputs are never written
            if (piece < n) v = *reinterpret_cast<const uint2*>((which ? face : pred) + piece * padded + k0 + 4 * q);
            *reinterpret_cast<uint2*>(&lds[which][r * PD_ROW + 4 * q]) = v;
        }
        __syncthreads();
        for (int q = 0; q < items; ++q) {
            const uint2 b = *reinterpret_cast<const uint2*>(&lds[1][tx * PD_ROW + 4 * q]);
#pragma unroll
            for (int a = 0; a < PD_PER_THREAD; ++a) {
                const uint2 p = *reinterpret_cast<const uint2*>(&lds[0][(ty + 8 * a) * PD_ROW + 4 * q]);
                acc[a] = pp::sad2(p.y, b.y, pp::sad2(p.x, b.x, acc[a]));
            }
        }
        __syncthreads();
    }
    const int64_t j = j0 + tx;
#pragma unroll
    for (int a = 0; a < PD_PER_THREAD; ++a) {
        const int64_t i = i0 + ty + 8 * a;
        if (i < n && j < n) dq[((int64_t)s * n + i) * n + j] = i == j ? pp::DQ_UNSET : (int)acc[a];
    }
}

// ---- distances, type 2: all 16 side pairings -------------------------------------------------------------------------------------------
// Pass 1: the strips of a piece, 4 sides x 3 kinds.  strips[0][s][i] is the prediction of side s of piece i, strips[1][s][i] its border
// and strips[2][s][i] its border read from the far end (puzzle_pixels.h: pairing_reversed), `padded` uint16 each.
__global__ void __launch_bounds__(PP_THREADS)
puzzle_strips2_kernel(const uint8_t* __restrict__ pieces, int64_t n, int We, int padded, uint16_t* __restrict__ strips) {
    const int64_t idx = (int64_t)blockIdx.x * PP_THREADS + threadIdx.x;
    const int64_t per_kind = 4 * n * padded;
    if (idx >= 3 * per_kind) return;
    const int kind = (int)(idx / per_kind);
    const int64_t rem = idx - kind * per_kind;
    const int k = (int)(rem % padded);
    const int64_t si = rem / padded;                            // s * n + i
    const int s = (int)(si / n);
    const uint8_t* piece = pieces + (si - s * n) * We * We * pp::CHANNELS;
    strips[idx] = kind == 0 ? pp::strip_prediction(piece, We, s, k)
                            : (kind == 1 ? pp::strip_border(piece, We, s, k) : pp::strip_border_reversed(piece, We, s, k));
}

// Pass 2: a workgroup owns the PD_TILE x PD_TILE block (i0.., j0..) of one side si of i and all four sides sj of j.  Per stage it puts the
// predictions of its 32 i and, for each sj, the border strips of its 32 j in the order the pairing (si, sj) reads them into LDS - rows
// laid out as in the type-1 kernel, so the reads stay conflict-free - and thread (ty, tx) accumulates the 4 x 4 outputs
// (i0 + ty + 8 a, j0 + tx, sj) with v_sad_u16.  The four sj of one (i, j) leave as one 16-byte store.
__global__ void __launch_bounds__(PP_THREADS)
puzzle_pixel_distances2_kernel(const uint16_t* __restrict__ strips, int64_t n, int padded, int* __restrict__ dq2) {
    __shared__ __attribute__((aligned(16))) uint16_t lds[5][PD_TILE * PD_ROW];       // [0]: predictions, [1 + sj]: borders
    const int si = blockIdx.z;
    const int64_t i0 = (int64_t)blockIdx.y * PD_TILE, j0 = (int64_t)blockIdx.x * PD_TILE;
    const int tx = threadIdx.x % PD_TILE, ty = threadIdx.x / PD_TILE;
    const int64_t per_side = n * padded, per_kind = 4 * per_side;
    uint32_t acc[PD_PER_THREAD][4];
#pragma unroll
    for (int a = 0; a < PD_PER_THREAD; ++a)
#pragma unroll
        for (int sj = 0; sj < 4; ++sj) acc[a][sj] = 0u;
    for (int k0 = 0; k0 < padded; k0 += PD_STAGE) {
        const int items = (padded - k0 < PD_STAGE ? padded - k0 : PD_STAGE) / 4;       // 8-byte items of this stage, per row
        for (int idx = threadIdx.x; idx < 5 * PD_TILE * (PD_STAGE / 4); idx += PP_THREADS) {
            const int which = idx / (PD_TILE * (PD_STAGE / 4)), rem = idx % (PD_TILE * (PD_STAGE / 4));
            const int r = rem / (PD_STAGE / 4), q = rem % (PD_STAGE / 4);
            if (q >= items) continue;
            const int64_t piece = (which ? j0 : i0) + r;
            const uint16_t* src = which == 0 ? strips + si * per_side
                                             : strips + (pp::pairing_reversed(si, which - 1) ? 2 : 1) * per_kind + (which - 1) * per_side;
            uint2 v = make_uint2(0u, 0u);                       // rows past n: zeros, their outputs are never written
            if (piece < n) v = *reinterpret_cast<const uint2*>(src + piece * padded + k0 + 4 * q);
            *reinterpret_cast<uint2*>(&lds[which][r * PD_ROW + 4 * q]) = v;
        }
        __syncthreads();
        for (int q = 0; q < items; ++q) {
            uint2 b[4];
#pragma unroll
            for (int sj = 0; sj < 4; ++sj) b[sj] = *reinterpret_cast<const uint2*>(&lds[1 + sj][tx * PD_ROW + 4 * q]);
#pragma unroll
            for (int a = 0; a < PD_PER_THREAD; ++a) {
                const uint2 p = *reinterpret_cast<const uint2*>(&lds[0][(ty + 8 * a) * PD_ROW + 4 * q]);
#pragma unroll
                for (int sj = 0; sj < 4; ++sj) acc[a][sj] = pp::sad2(p.y, b[sj].y, pp::sad2(p.x, b[sj].x, acc[a][sj]));
            }
        }
        __syncthreads();
    }
    const int64_t j = j0 + tx;
#pragma unroll
    for (int a = 0; a < PD_PER_THREAD; ++a) {
        const int64_t i = i0 + ty + 8 * a;
        if (i >= n || j >= n) continue;
        const int4 out = i == j ? make_int4(pp::DQ_UNSET, pp::DQ_UNSET, pp::DQ_UNSET, pp::DQ_UNSET)
                                : make_int4((int)acc[a][0], (int)acc[a][1], (int)acc[a][2], (int)acc[a][3]);
        *reinterpret_cast<int4*>(dq2 + (((int64_t)si * n + i) * n + j) * 4) = out;
    }
}

// ---- board: one thread per output pixel, a gather ------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PP_THREADS)
puzzle_assemble_kernel(const uint8_t* __restrict__ pieces, int64_t n, int We, int P, const int* __restrict__ cells, int64_t rows,
                       int64_t cols, int marker, uint8_t* __restrict__ board) {
    const int64_t width = cols * P;
    const int64_t idx = (int64_t)blockIdx.x * PP_THREADS + threadIdx.x;
    if (idx >= rows * P * width) return;
    const int64_t Y = idx / width, X = idx - Y * width;
#pragma unroll
    for (int c = 0; c < pp::CHANNELS; ++c) board[idx * pp::CHANNELS + c] = pp::board_byte(pieces, n, We, P, cells, cols, marker, Y, X, c);
}

__global__ void __launch_bounds__(PP_THREADS)
puzzle_assemble2_kernel(const uint8_t* __restrict__ pieces, int64_t n, int We, int P, const int* __restrict__ cells,
                        const int* __restrict__ rotations, int64_t rows, int64_t cols, int marker, uint8_t* __restrict__ board) {
    const int64_t width = cols * P;
    const int64_t idx = (int64_t)blockIdx.x * PP_THREADS + threadIdx.x;
    if (idx >= rows * P * width) return;
    const int64_t Y = idx / width, X = idx - Y * width;
#pragma unroll
    for (int c = 0; c < pp::CHANNELS; ++c)
        board[idx * pp::CHANNELS + c] = pp::board_byte_rotated(pieces, n, We, P, cells, rotations, cols, marker, Y, X, c);
}

bool sizes_ok(int64_t n, int We) { return n >= 1 && We >= 2; }
bool sizes_supported(int64_t n, int We) { return n <= pp::MAX_PIECES && We <= pp::MAX_ERODED; }
unsigned blocks_for(int64_t items) { return (unsigned)ceil_div64(items, PP_THREADS); }

}  // namespace

extern "C" int vited_puzzle_cut(const uint8_t* image, int64_t height, int64_t width, int piece_width, int eroded_width,
                                const int* order, int64_t n, uint8_t* pieces, void* stream) {
    if (!image || !pieces || height < 1 || width < 1 || !sizes_ok(n, eroded_width) || piece_width < eroded_width) return VITED_ERR_BAD_ARG;
    if (!sizes_supported(n, eroded_width) || height > INT32_MAX || width > INT32_MAX) return VITED_ERR_UNSUPPORTED;
    const pp::Cut g = pp::cut_geometry(height, width, piece_width, eroded_width);
    if (g.rows * g.cols != n) return VITED_ERR_BAD_ARG;
    const int64_t items = n * eroded_width * eroded_width;
    if (ceil_div64(items, PP_THREADS) > INT32_MAX) return VITED_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(puzzle_cut_kernel, dim3(blocks_for(items)), dim3(PP_THREADS), 0, static_cast<hipStream_t>(stream), image, g, order, n,
                       pieces);
    return vited_check_launch();
}

extern "C" int vited_puzzle_resize_pieces(const uint8_t* pieces, int64_t n, int eroded_width, int size, uint8_t* out, void* stream) {
    if (!pieces || !out || !sizes_ok(n, eroded_width) || size < eroded_width) return VITED_ERR_BAD_ARG;
    if (size > PP_MAX_SIZE || n > INT32_MAX) return VITED_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(puzzle_resize_kernel, dim3((unsigned)n), dim3(PP_THREADS), 0, static_cast<hipStream_t>(stream), pieces, eroded_width,
                       size, out);
    return vited_check_launch();
}

extern "C" int64_t vited_puzzle_pixel_distances_workspace_bytes(int64_t n, int eroded_width) {
    if (!sizes_ok(n, eroded_width) || n < 2 || !sizes_supported(n, eroded_width)) return -1;
    return 2 * 4 * n * (int64_t)pp::strip_padded(eroded_width) * (int64_t)sizeof(uint16_t);
}

extern "C" int vited_puzzle_pixel_distances(const uint8_t* pieces, int64_t n, int eroded_width, int* dq, void* workspace,
                                            int64_t workspace_bytes, void* stream) {
    if (!pieces || !dq || !workspace || !sizes_ok(n, eroded_width) || n < 2) return VITED_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0 || reinterpret_cast<uintptr_t>(dq) % 4 != 0) return VITED_ERR_BAD_ARG;
    if (!sizes_supported(n, eroded_width)) return VITED_ERR_UNSUPPORTED;
    if (workspace_bytes < vited_puzzle_pixel_distances_workspace_bytes(n, eroded_width)) return VITED_ERR_WORKSPACE;
    const int padded = pp::strip_padded(eroded_width);
    const int64_t values = 2 * 4 * n * padded;
    if (ceil_div64(values, PP_THREADS) > INT32_MAX) return VITED_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint16_t* strips = static_cast<uint16_t*>(workspace);
    hipLaunchKernelGGL(puzzle_strips_kernel, dim3(blocks_for(values)), dim3(PP_THREADS), 0, st, pieces, n, eroded_width, padded, strips);
    const unsigned tiles = (unsigned)ceil_div64(n, PD_TILE);
    hipLaunchKernelGGL(puzzle_pixel_distances_kernel, dim3(tiles, tiles, 4), dim3(PP_THREADS), 0, st, strips, n, padded, dq);
    return vited_check_launch();
}

extern "C" int vited_puzzle_assemble(const uint8_t* pieces, int64_t n, int eroded_width, int piece_width, const int* cells, int64_t rows,
                                     int64_t cols, int marker, uint8_t* board, void* stream) {
    if (!pieces || !cells || !board || !sizes_ok(n, eroded_width) || piece_width < eroded_width) return VITED_ERR_BAD_ARG;
    if (rows < 1 || cols < 1 || rows > n || cols > n || marker > 0xffffff) return VITED_ERR_BAD_ARG;
    if (marker >= 0 && (piece_width - eroded_width) / 2 < 1) return VITED_ERR_BAD_ARG;       // the frame needs a pixel of padding
    if (!sizes_supported(n, eroded_width)) return VITED_ERR_UNSUPPORTED;
    if (rows * cols != n) return VITED_ERR_BAD_ARG;
    const int64_t pixels = rows * piece_width * cols * piece_width;
    if (ceil_div64(pixels, PP_THREADS) > INT32_MAX) return VITED_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(puzzle_assemble_kernel, dim3(blocks_for(pixels)), dim3(PP_THREADS), 0, static_cast<hipStream_t>(stream), pieces, n,
                       eroded_width, piece_width, cells, rows, cols, marker, board);
    return vited_check_launch();
}

// ---- type 2 (pieces of unknown rotation) ---------------------------------------------------------------------------------------------
extern "C" int64_t vited_puzzle_pixel_distances2_workspace_bytes(int64_t n, int eroded_width) {
    if (!sizes_ok(n, eroded_width) || n < 2 || !sizes_supported(n, eroded_width)) return -1;
    return 3 * 4 * n * (int64_t)pp::strip_padded(eroded_width) * (int64_t)sizeof(uint16_t);
}

extern "C" int vited_puzzle_pixel_distances2(const uint8_t* pieces, int64_t n, int eroded_width, int* dq2, void* workspace,
                                             int64_t workspace_bytes, void* stream) {
    if (!pieces || !dq2 || !workspace || !sizes_ok(n, eroded_width) || n < 2) return VITED_ERR_BAD_ARG;
    if (reinterpret_cast<uintptr_t>(workspace) % 8 != 0 || reinterpret_cast<uintptr_t>(dq2) % 16 != 0) return VITED_ERR_BAD_ARG;
    if (!sizes_supported(n, eroded_width)) return VITED_ERR_UNSUPPORTED;
    if (workspace_bytes < vited_puzzle_pixel_distances2_workspace_bytes(n, eroded_width)) return VITED_ERR_WORKSPACE;
    const int padded = pp::strip_padded(eroded_width);
    const int64_t values = 3 * 4 * n * padded;
    if (ceil_div64(values, PP_THREADS) > INT32_MAX) return VITED_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint16_t* strips = static_cast<uint16_t*>(workspace);
    hipLaunchKernelGGL(puzzle_strips2_kernel, dim3(blocks_for(values)), dim3(PP_THREADS), 0, st, pieces, n, eroded_width, padded, strips);
    const unsigned tiles = (unsigned)ceil_div64(n, PD_TILE);
    hipLaunchKernelGGL(puzzle_pixel_distances2_kernel, dim3(tiles, tiles, 4), dim3(PP_THREADS), 0, st, strips, n, padded, dq2);
    return vited_check_launch();
}

extern "C" int vited_puzzle_assemble2(const uint8_t* pieces, int64_t n, int eroded_width, int piece_width, const int* cells,
                                      const int* rotations, int64_t rows, int64_t cols, int marker, uint8_t* board, void* stream) {
    if (!pieces || !cells || !rotations || !board || !sizes_ok(n, eroded_width) || piece_width < eroded_width) return VITED_ERR_BAD_ARG;
    if (rows < 1 || cols < 1 || rows > n || cols > n || marker > 0xffffff) return VITED_ERR_BAD_ARG;
    if (marker >= 0 && (piece_width - eroded_width) / 2 < 1) return VITED_ERR_BAD_ARG;       // the frame needs a pixel of padding
    if (!sizes_supported(n, eroded_width)) return VITED_ERR_UNSUPPORTED;
    if (rows * cols != n) return VITED_ERR_BAD_ARG;
    const int64_t pixels = rows * piece_width * cols * piece_width;
    if (ceil_div64(pixels, PP_THREADS) > INT32_MAX) return VITED_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(puzzle_assemble2_kernel, dim3(blocks_for(pixels)), dim3(PP_THREADS), 0, static_cast<hipStream_t>(stream), pieces, n,
                       eroded_width, piece_width, cells, rotations, rows, cols, marker, board);
    return vited_check_launch();
}

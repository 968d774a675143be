// Device ray loader: one shuffled training batch drawn from the 22-column ray table that already lives in HBM (raytable.ray_table), replacing the
// reference's per-step host path - two DataLoader(shuffle=True, num_workers=4) collating batch_size single-row __getitem__ calls
// (mg_run_NeRF.py:74-84,229-264; NN_loaders/mg_Color_Loader.py:94-102), t.rand(4) per sun-check ray (NN_loaders/mg_SC_loader.py:17-21), upload.
//   loader_draw_kernel      row i of the batch <- table[perm_epoch(((batch_in_epoch * world) + rank) * B + i)], split into the fields get_loss reads
//                           (Net_tool.data_to_dict, mg_run_NeRF.py:122-133), + the row index, + the random sun-check ray of SC_loader.__getitem__
//   loader_advance_kernel   <<<1,1>>> behind the draw on the same stream: draws + 1, batch_in_epoch + 1, wrap into the next epoch
// The position is READ FROM DEVICE MEMORY (state = {epoch, batch_in_epoch, draws, reserved}, int64), never passed as a launch argument: a hipGraph that
// holds the two launches as kernel nodes draws a new batch at every replay.  The advance is its own launch so that no block of the draw races with the
// writer.  HBM-bound and tiny (4096 rows: 360 KB read, 360 KB written); 32 lanes per row - lanes 0..21 move the row's 22 floats (one 88-byte read per
// row, the field writes contiguous over neighbouring rows), lanes 22..27 the six coordinates of the sun-check ray, lane 28 the row index.  Every lane
// derives the row index itself (integer work of a few hundred operations; no cross-lane traffic, no early exit to guard).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "loader_common.h"

namespace snerf {

__global__ __launch_bounds__(256) void loader_draw_kernel(const LoaderArgs A) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = t >> 5;
    const int c = (int)(t & 31);
    if (i >= A.rows || c > 28) return;
    const int64_t epoch = A.state[0], bie = A.state[1], draws = A.state[2];
    if (bie < 0 || bie >= A.batches_per_epoch) return;              // memory safety only: a state nobody should have written
    const int64_t p = (bie * A.world + A.rank) * A.batch + i;
    if (p >= A.n_rows) return;                                      // (a short last batch whose size the host got wrong reads nothing out of bounds)
    if (c >= 22 && c < 28) {                                        // SC_loader.__getitem__: rands[0] * dx + x, rands[1] * dy + y, bounds[2, 1] | ... bounds[2, 0]
        const int k = c - 22, ax = k % 3;
        float* out = k < 3 ? A.sc_top : A.sc_bot;
        if (!out) return;
        float v = k < 3 ? A.z_hi : A.z_lo;
        if (ax < 2) {
            uint32_t w[4];
            loader_sc_words(A.seed, (uint64_t)draws, (uint32_t)A.rank, (uint32_t)i, w);
            const float u = loader_uniform(w[(k < 3 ? 0 : 2) + ax]);
            v = __fadd_rn(__fmul_rn(u, ax ? A.dy : A.dx), ax ? A.y0 : A.x0);
        }
        out[i * 3 + ax] = v;
        return;
    }
    const LoaderKeys K = loader_keys(A.seed, (uint64_t)epoch);
    const int64_t r = loader_perm(p, A.n_rows, A.bits, K);
    if (c == 28) {
        if (A.index) A.index[i] = r;
        return;
    }
    float* out;
    int w, j;
    if (c < 2) { out = A.img_pt; w = 2; j = c; }
    else if (c < 5) { out = A.top; w = 3; j = c - 2; }
    else if (c < 8) { out = A.bot; w = 3; j = c - 5; }
    else if (c < 11) { out = A.view; w = 3; j = c - 8; }
    else if (c < 14) { out = A.sun; w = 3; j = c - 11; }
    else if (c < 18) { out = A.time; w = 4; j = c - 14; }
    else if (c < 19) { out = A.weight; w = 1; j = 0; }
    else { out = A.gt; w = 3; j = c - 19; }
    if (out) out[i * w + j] = A.table[r * kLoaderCols + c];
}

__global__ void loader_advance_kernel(int64_t* state, int64_t batches_per_epoch) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t epoch = state[0], bie = state[1] + 1;
    if (bie >= batches_per_epoch) { bie = 0; epoch += 1; }
    state[0] = epoch;
    state[1] = bie;
    state[2] = state[2] + 1;
}

hipError_t launch_loader_draw(const LoaderArgs& a, hipStream_t st) {
    if (a.rows <= 0) return hipSuccess;
    const int64_t blocks = (a.rows * 32 + 255) / 256;
    hipLaunchKernelGGL(loader_draw_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_loader_advance(int64_t* state, int64_t batches_per_epoch, hipStream_t st) {
    hipLaunchKernelGGL(loader_advance_kernel, dim3(1), dim3(1), 0, st, state, batches_per_epoch);
    return hipGetLastError();
}

}  // namespace snerf

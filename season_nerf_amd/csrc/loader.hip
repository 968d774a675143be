// Device ray loader: one shuffled training batch drawn from the 22-column ray table that already lives in HBM (raytable.ray_table), replacing the
// reference's per-step host path - two DataLoader(shuffle=True, num_workers=4) collating batch_size single-row __getitem__ calls
// (mg_run_NeRF.py:74-84,229-264; NN_loaders/mg_Color_Loader.py:94-102), t.rand(4) per sun-check ray (NN_loaders/mg_SC_loader.py:17-21), upload.
//   loader_draw_kernel      row i of the batch <- table[perm_epoch(((batch_in_epoch * world) + rank) * B + i)], split into the fields get_loss reads
//                           (Net_tool.data_to_dict, mg_run_NeRF.py:122-133), + the row index, + the random sun-check ray of SC_loader.__getitem__
//   loader_advance_kernel   <<<1,1>>> behind the draw on the same stream: draws + 1, batch_in_epoch + 1, wrap into the next epoch
//   step_inputs_draw_kernel / step_inputs_advance_kernel   the same pattern for what the step draws besides its batch (further down)
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

// ---- per-step training inputs -----------------------------------------------------------------------------------------------------------------------
// What trainer.GraphedTrainStep._load draws on the host between two replays, drawn here instead: the random sun rays of the solar-correction loss
// (Eval_Tools_2.py:72-108), the jitter of both sampling passes (misc.py:236-241), and row `step` of the schedule table (Adam's six scalars, the DSM prior's
// trust factor, the second optimiser's learning rate).  state = {draws, step, reserved, reserved} in device memory, advanced by a one-thread kernel behind
// the draw, as the loader's: two kernel nodes in a captured step.  One thread per ray (two Philox blocks, the float64 arithmetic of
// training._angles_to_local_vecs operation by operation - explicit _rn intrinsics: the four-term sums cancel ~1e4 against O(1), nothing may be contracted),
// then one per sample, then eight for the table row.  Word assignment: loader_common.h.
__global__ __launch_bounds__(256) void step_inputs_draw_kernel(const StepInputsArgs A) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t draws = (uint64_t)A.state[0];
    if (t < A.n_rays) {
        const int64_t i = t;
        uint32_t w[4], w1[4];
        step_inputs_words(A.seed, draws, A.rank, 0, (uint32_t)i, w);
        const float sx = __fadd_rn(__fmul_rn(2.0f, loader_uniform(w[2])), -1.0f), sy = __fadd_rn(__fmul_rn(2.0f, loader_uniform(w[3])), -1.0f);
        if (A.starts) { A.starts[i * 3] = sx; A.starts[i * 3 + 1] = sy; A.starts[i * 3 + 2] = 1.0f; }
        if (A.ends || A.vec) {
            const double k2m32 = 2.3283064365386963e-10, d2r = 3.14159265358979323846 / 180.0, r2d = 180.0 / 3.14159265358979323846;
            const double az = __dadd_rn(__dmul_rn(__dmul_rn((double)w[0], k2m32), 360.0), -180.0);
            const double el = __dadd_rn(__dmul_rn(__dmul_rn((double)w[1], k2m32), 89.0), 1.0);
            const double azr = __dmul_rn(az, d2r), elr = __dmul_rn(el, d2r);
            double Y = cos(azr), X = sin(azr);
            const double xy2 = __dadd_rn(__dmul_rn(X, X), __dmul_rn(Y, Y));
            double Z = __dmul_rn(tan(elr), sqrt(xy2));
            const double nrm = __ddiv_rn(sqrt(__dadd_rn(xy2, __dmul_rn(Z, Z))), 1000.0);
            X = __ddiv_rn(X, nrm); Y = __ddiv_rn(Y, nrm); Z = __ddiv_rn(Z, nrm);
            const double P0 = __dadd_rn(A.wc[0], __dmul_rn(__ddiv_rn(Y, 1000.0 * 6378.137), r2d));
            const double P1 = __dadd_rn(A.wc[1], __dmul_rn(__ddiv_rn(X, A.lon_scale), r2d));
            const double P2 = __dadd_rn(A.wc[2], Z);
            double v[3];
            for (int r = 0; r < 3; ++r) {
                const double* h = A.H + r * 4;
                v[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(h[0], P0), __dmul_rn(h[1], P1)), __dmul_rn(h[2], P2)), h[3]);
            }
            const double len = sqrt(__dadd_rn(__dadd_rn(__dmul_rn(v[0], v[0]), __dmul_rn(v[1], v[1])), __dmul_rn(v[2], v[2])));
            for (int r = 0; r < 3; ++r) v[r] = __ddiv_rn(v[r], len);
            if (A.vec) { A.vec[i * 3] = (float)v[0]; A.vec[i * 3 + 1] = (float)v[1]; A.vec[i * 3 + 2] = (float)v[2]; }
            if (A.ends) {
                const float s3[3] = {sx, sy, 1.0f};
                for (int r = 0; r < 3; ++r) A.ends[i * 3 + r] = (float)__dsub_rn((double)s3[r], __dmul_rn(2.0, __ddiv_rn(v[r], v[2])));
            }
        }
        if (A.times) {
            step_inputs_words(A.seed, draws, A.rank, 1, (uint32_t)i, w1);
            const float two_pi = 6.2831854820251465f;                   // fp32(2 pi)
            const double a0 = (double)__fmul_rn(loader_uniform(w1[0]), two_pi), a1 = (double)__fmul_rn(loader_uniform(w1[1]), two_pi);
            A.times[i * 4] = (float)cos(a0); A.times[i * 4 + 1] = (float)sin(a0); A.times[i * 4 + 2] = (float)cos(a1); A.times[i * 4 + 3] = (float)sin(a1);
        }
        return;
    }
    const int64_t s = t - A.n_rays;
    if (s < A.n_samples) {
        if (!A.base || (!A.tv_image && !A.tv_solar)) return;
        uint32_t w[4];
        step_inputs_words(A.seed, draws, A.rank, 2, (uint32_t)s, w);
        const float b = A.base[s];
        if (A.tv_image) A.tv_image[s] = __fadd_rn(b, __fmul_rn(A.inv_s, loader_uniform(w[0])));
        if (A.tv_solar) A.tv_solar[s] = __fadd_rn(b, __fmul_rn(A.inv_s, loader_uniform(w[1])));
        return;
    }
    const int64_t c = s - A.n_samples;
    if (c >= 8 || !A.table || A.table_rows < 1) return;
    int64_t row = A.state[1];
    row = row < 0 ? 0 : (row >= A.table_rows ? A.table_rows - 1 : row);       // past the last row: the last row (Python refuses before that)
    const float x = A.table[row * 8 + c];
    if (c < 6) { if (A.hyper) A.hyper[c] = x; }
    else if (c == 6) { if (A.trust) A.trust[0] = x; }
    else if (A.lr2) A.lr2[0] = x;
}

__global__ void step_inputs_advance_kernel(int64_t* state) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    state[0] = state[0] + 1;
    state[1] = state[1] + 1;
}

hipError_t launch_step_inputs_draw(const StepInputsArgs& a, hipStream_t st) {
    const int64_t threads = a.n_rays + a.n_samples + 8;
    hipLaunchKernelGGL(step_inputs_draw_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, a);
    return hipGetLastError();
}
hipError_t launch_step_inputs_advance(int64_t* state, hipStream_t st) {
    hipLaunchKernelGGL(step_inputs_advance_kernel, dim3(1), dim3(1), 0, st, state);
    return hipGetLastError();
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

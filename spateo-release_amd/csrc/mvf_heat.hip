// Digitization: the two Jacobi relaxations of the heat equation of spateo/digitization/utils.py, whole loops on the device.
// gfx950 only, float64 only, no floating-point atomics: two calls give equal bits.
//
//   mvf_heat_grid   `domain_heat_eqn_solver` (utils.py:464-524): the 5-point average on the H x W raster of a slice,
//       new[y, x] = 0.25 * (((old[y, x+1] + old[y, x-1]) + old[y+1, x]) + old[y-1, x])      (the reference's left-to-right order)
//     for every pixel that is not FIXED (field_border != 0, or on the array's outer rows / columns); a fixed pixel keeps the
//     value of `init`.  The sweep covers the whole array, pixels outside the mask included (a border need not be closed).
//     Per sweep S1 = sum (new - old)^2 mask and S0 = sum old^2 mask (`effective_L2_error` normalises by its SECOND argument and
//     the call passes the old field there), err = sqrt(S1 / S0); the loop goes on exactly while err > max_err && itr <= max_itr,
//     so a NaN err ends it and floor(max_itr) + 1 sweeps run at most.  The result is field * mask.
//   mvf_heat_graph  `digitize_general` (utils.py:527-575): new_j = sum_i old_i A_ij over the CSC column of node j, added one
//     after the other in ascending i from 0; a node with fixed_value != 0 then takes fixed_value (a boundary given heat 0 is
//     not held - the reference's np.where).  S1 = sum (new - old)^2, S0 = sum new^2 over all nodes.
//
// Grid kernel: a workgroup owns a 32 x 64 tile and keeps it with a halo of up to 8 pixels in LDS (48 x 80 float64 = 30 KB, so
// five workgroups share a CU's 160 KB); one launch runs `steps` sweeps there, 1 <= steps <= 8.  A lane holds the same 15 cells
// in every sweep: it reads their neighbours, all lanes meet, it writes.  Sweep s computes the cells within steps - 1 - s of the
// tile, whose neighbours the sweep before left valid, so a halo cell goes through exactly the operations its owner applies and
// carries the same bits.  steps == 1 is the plain one-sweep kernel (a halo of one pixel is loaded).  Each sweep leaves one pair
// of partial sums per workgroup, over the pixels it owns, added in lane order; heat_finalize_kernel adds the pairs in workgroup
// order, sweep by sweep, finds the first sweep that meets the stop rule and raises the flag of the status block.  Every launch
// after that reads the flag and returns at once, which keeps the buffer that held the field before the stopping batch: when the
// stop falls inside a batch the host runs that batch again from it, with steps = t* + 1.  The host reads the status block every
// HEAT_POLL batches.
//
// No grid-wide barrier and no workgroup that waits on another one: sweeps are ordered by kernel boundaries alone.
#include <cstring>

#include "mvf_common.h"

namespace mvf {

constexpr int HEAT_T = MVF_HEAT_MAX_STEPS;         // sweeps per launch at most == pixels of halo
constexpr int HEAT_TX = 64, HEAT_TY = 32;           // the tile a workgroup owns
constexpr int HEAT_LX = HEAT_TX + 2 * HEAT_T;       // 80
constexpr int HEAT_LY = HEAT_TY + 2 * HEAT_T;       // 48
constexpr int HEAT_THREADS = 256;
constexpr int HEAT_PER = HEAT_LX * HEAT_LY / HEAT_THREADS;  // 15 cells per lane
static_assert(HEAT_PER * HEAT_THREADS == HEAT_LX * HEAT_LY && HEAT_PER <= 16 && HEAT_T < 15, "heat tile");
constexpr int HEAT_POLL = 16;                       // batches between two reads of the status block

struct HeatStatus {        // 64 bytes on the device, read back whole
    long long done;        // the stop rule was met: later launches do nothing
    long long sweeps;      // sweeps counted so far (itr of the reference)
    long long stop_t;      // the sweep inside its batch at which the loop stopped
    long long batch;       // that batch
    long long hit;         // err > max_err still held there: the sweep budget ended the loop
    double err;            // the last err
    long long pad[2];
};

__global__ __launch_bounds__(HEAT_THREADS) void heat_status_init_kernel(HeatStatus* st) {
    if (threadIdx.x == 0) {
        st->done = 0, st->sweeps = 0, st->stop_t = -1, st->batch = -1, st->hit = 0, st->err = 1.0;
        st->pad[0] = st->pad[1] = 0;
    }
}

// field = init; fixed = border != 0 or on the outer rows / columns
__global__ __launch_bounds__(HEAT_THREADS) void heat_grid_prep_kernel(const double* __restrict__ init, const double* __restrict__ border,
                                                                      int64_t H, int64_t W, double* __restrict__ field,
                                                                      uint8_t* __restrict__ fixed) {
    const int64_t g = (int64_t)blockIdx.x * HEAT_THREADS + threadIdx.x;
    if (g >= H * W) return;
    const int64_t y = g / W, x = g - y * W;
    field[g] = init[g];
    fixed[g] = (border[g] != 0.0 || y == 0 || y == H - 1 || x == 0 || x == W - 1) ? 1 : 0;
}

__global__ __launch_bounds__(HEAT_THREADS) void heat_grid_mask_kernel(const double* __restrict__ field, const double* __restrict__ mask,
                                                                      int64_t total, double* __restrict__ out) {
    const int64_t g = (int64_t)blockIdx.x * HEAT_THREADS + threadIdx.x;
    if (g < total) out[g] = field[g] * mask[g];
}

// `steps` sweeps of the tile of this workgroup: src -> dst (owned pixels), part[(s * nwg + wg) * 2 + {0, 1}] = this workgroup's
// S1, S0 of sweep s.  status == NULL: run whatever the flag says (the host's repeat of the stopping batch).
__global__ __launch_bounds__(HEAT_THREADS) void heat_grid_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                                 const uint8_t* __restrict__ fixed, const double* __restrict__ mask,
                                                                 int H, int W, int steps, const HeatStatus* __restrict__ status,
                                                                 double* __restrict__ part) {
    __shared__ double f[HEAT_LX * HEAT_LY];
    __shared__ double red[HEAT_T * 2 * (HEAT_THREADS / 64)];
    if (status && status->done) return;  // (the same for every lane of every workgroup: written by an earlier kernel)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int x0 = (int)blockIdx.x * HEAT_TX - HEAT_T, y0 = (int)blockIdx.y * HEAT_TY - HEAT_T;
    // per cell k of this lane: ring (4 bits) = its distance from the tile, 15 for a cell that is never computed (fixed, outside
    // the array, or further out than `steps`); own (1 bit) = a pixel of the tile inside the array; mk = its mask weight
    unsigned long long ring = 0;
    unsigned own = 0;
    double mk[HEAT_PER];
#pragma unroll
    for (int k = 0; k < HEAT_PER; ++k) {
        const int idx = tid + k * HEAT_THREADS;
        const int ly = idx / HEAT_LX, lx = idx - ly * HEAT_LX;
        const int gy = y0 + ly, gx = x0 + lx;
        const int dy = ly < HEAT_T ? HEAT_T - ly : (ly >= HEAT_T + HEAT_TY ? ly - (HEAT_T + HEAT_TY - 1) : 0);
        const int dx = lx < HEAT_T ? HEAT_T - lx : (lx >= HEAT_T + HEAT_TX ? lx - (HEAT_T + HEAT_TX - 1) : 0);
        const int d = max(dx, dy);
        double v = 0.0, m = 0.0;
        unsigned long long code = 15;
        if (gy >= 0 && gy < H && gx >= 0 && gx < W && d <= steps) {
            const int64_t g = (int64_t)gy * W + gx;
            v = src[g];
            if (!fixed[g]) code = (unsigned long long)d;
            if (d == 0) {
                m = mask[g];
                own |= 1u << k;
            }
        }
        ring |= code << (4 * k);
        mk[k] = m;
        f[idx] = v;
    }
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < steps; ++s) {
        const int lim = steps - 1 - s;
        double nv[HEAT_PER];
        double a1 = 0.0, a0 = 0.0;
#pragma unroll
        for (int k = 0; k < HEAT_PER; ++k) {
            const int idx = tid + k * HEAT_THREADS;
            const bool compute = (int)((ring >> (4 * k)) & 15) <= lim;  // (never a cell on the edge of the LDS image: ring <= 7)
            double old = 0.0, nw = 0.0;
            if (compute || ((own >> k) & 1u)) old = f[idx];
            nw = old;
            if (compute) nw = 0.25 * (((f[idx + 1] + f[idx - 1]) + f[idx + HEAT_LX]) + f[idx - HEAT_LX]);
            nv[k] = nw;
            if ((own >> k) & 1u) {
                const double df = nw - old;
                a1 += (df * df) * mk[k];
                a0 += (old * old) * mk[k];
            }
        }
        __syncthreads();  // every neighbour is read
#pragma unroll
        for (int k = 0; k < HEAT_PER; ++k)
            if ((int)((ring >> (4 * k)) & 15) <= lim) f[tid + k * HEAT_THREADS] = nv[k];
        a1 = wave_sum(a1), a0 = wave_sum(a0);
        if (lane == 0) red[(s * 2 + 0) * (HEAT_THREADS / 64) + wv] = a1, red[(s * 2 + 1) * (HEAT_THREADS / 64) + wv] = a0;
        __syncthreads();  // every cell is written
    }
    if (tid < 2 * steps) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < HEAT_THREADS / 64; ++w) t += red[tid * (HEAT_THREADS / 64) + w];
        const int64_t nwg = (int64_t)gridDim.x * gridDim.y, wg = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
        part[((int64_t)(tid >> 1) * nwg + wg) * 2 + (tid & 1)] = t;
    }
#pragma unroll
    for (int k = 0; k < HEAT_PER; ++k) {
        if ((own >> k) & 1u) {
            const int idx = tid + k * HEAT_THREADS;
            const int ly = idx / HEAT_LX, lx = idx - ly * HEAT_LX;
            dst[(int64_t)(y0 + ly) * W + (x0 + lx)] = f[idx];
        }
    }
}

// One sweep of the graph: a lane owns a node and adds its column in ascending row order.
__global__ __launch_bounds__(HEAT_THREADS) void heat_graph_kernel(const double* __restrict__ src, double* __restrict__ dst,
                                                                  const int64_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                                  const double* __restrict__ vals, const double* __restrict__ fixedv,
                                                                  int64_t n, const HeatStatus* __restrict__ status,
                                                                  double* __restrict__ part) {
    __shared__ double sm[HEAT_THREADS / 64];
    if (status->done) return;
    const int64_t j = (int64_t)blockIdx.x * HEAT_THREADS + threadIdx.x;
    double a1 = 0.0, a0 = 0.0;
    if (j < n) {
        double acc = 0.0;
        const int64_t hi = indptr[j + 1];
        for (int64_t e = indptr[j]; e < hi; ++e) acc += src[indices[e]] * vals[e];
        const double fv = fixedv[j];
        const double nw = (fv != 0.0) ? fv : acc;
        const double df = nw - src[j];
        a1 = df * df, a0 = nw * nw;
        dst[j] = nw;
    }
    const double s1 = block_sum<HEAT_THREADS>(a1, sm);
    const double s0 = block_sum<HEAT_THREADS>(a0, sm);
    if (threadIdx.x == 0) part[(int64_t)blockIdx.x * 2] = s1, part[(int64_t)blockIdx.x * 2 + 1] = s0;
}

// One workgroup: the partial sums of the `steps` sweeps of batch `batch`, in workgroup order; the stop rule sweep by sweep.
__global__ __launch_bounds__(HEAT_THREADS) void heat_finalize_kernel(const double* __restrict__ part, int64_t nwg, int steps,
                                                                     double max_err, double max_itr, long long batch,
                                                                     HeatStatus* __restrict__ st) {
    __shared__ double sm[HEAT_THREADS / 64];
    __shared__ int stop;
    const long long was_done = st->done;
    long long itr = st->sweeps;
    __syncthreads();  // (lane 0 writes the block below)
    if (was_done) return;
    for (int t = 0; t < steps; ++t) {
        double a1 = 0.0, a0 = 0.0;
        for (int64_t w = threadIdx.x; w < nwg; w += HEAT_THREADS) {
            a1 += part[((int64_t)t * nwg + w) * 2];
            a0 += part[((int64_t)t * nwg + w) * 2 + 1];
        }
        const double s1 = block_sum<HEAT_THREADS>(a1, sm);
        const double s0 = block_sum<HEAT_THREADS>(a0, sm);
        ++itr;
        if (threadIdx.x == 0) {
            const double err = sqrt(s1 / s0);
            const bool go_on = (err > max_err) && ((double)itr <= max_itr);
            st->err = err, st->sweeps = itr;
            if (!go_on) st->done = 1, st->stop_t = t, st->batch = batch, st->hit = (err > max_err) ? 1 : 0;
            stop = go_on ? 0 : 1;
        }
        __syncthreads();
        if (stop) return;
    }
}

// the sweeps the reference's `while err > max_err and itr <= max_itr` can run: 0 when the test fails before the first one
static inline long long heat_budget(double max_err, double max_itr) {
    if (!(1.0 > max_err) || !(0.0 <= max_itr)) return 0;
    if (max_itr >= 4.0e18) return (long long)4e18;
    return (long long)std::floor(max_itr) + 1;
}

static inline int64_t heat_grid_nwg(int64_t H, int64_t W) { return cdiv(H, HEAT_TY) * cdiv(W, HEAT_TX); }
// [status 256][field A][field B][partials HEAT_T x nwg x 2][fixed H x W bytes]
static inline size_t heat_grid_ws_bytes(int64_t H, int64_t W) {
    return 256 + (size_t)(2 * H * W + 2 * HEAT_T * heat_grid_nwg(H, W)) * 8 + align_up((size_t)(H * W), 8);
}
// [status 256][field A][field B][fixed_value n][partials nwg x 2][values nnz][indptr n + 1][indices nnz int32]
static inline size_t heat_graph_ws_bytes(int64_t n, int64_t nnz) {
    return 256 + (size_t)(3 * n + 2 * cdiv(n, HEAT_THREADS) + nnz + (n + 1)) * 8 + align_up((size_t)nnz * 4, 8);
}

static int heat_read_status(hipStream_t st, const HeatStatus* dev, HeatStatus* host) {
    MVF_CHECK_HIP(hipMemcpyAsync(host, dev, sizeof(HeatStatus), hipMemcpyDeviceToHost, st));
    MVF_CHECK_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // namespace mvf

using namespace mvf;

extern "C" size_t mvf_heat_grid_workspace_bytes(int64_t H, int64_t W) {
    if (H < 3 || W < 3 || H >= ((int64_t)1 << 20) || W >= ((int64_t)1 << 20)) return 0;
    return heat_grid_ws_bytes(H, W);
}

extern "C" int mvf_heat_grid(const double* init, const double* border, const double* mask, int64_t H, int64_t W, double max_err,
                             double max_itr, int block_steps, double* out, int64_t* sweeps, double* err, int* hit_max_itr,
                             void* workspace, size_t workspace_bytes, void* stream) {
    MVF_REQUIRE(H >= 3 && W >= 3 && H < ((int64_t)1 << 20) && W < ((int64_t)1 << 20),
                "mvf_heat_grid: bad shape (H=%lld, W=%lld; both at least 3 and below 2^20)", (long long)H, (long long)W);
    MVF_REQUIRE(block_steps >= 0 && block_steps <= HEAT_T, "mvf_heat_grid: bad block_steps %d (0: the dispatcher's choice, else 1 .. %d)",
                block_steps, HEAT_T);
    MVF_REQUIRE(init && border && mask && out && sweeps && err && hit_max_itr, "mvf_heat_grid: null pointer");
    MVF_REQUIRE(workspace, "mvf_heat_grid: null pointer (workspace)");
    MVF_REQUIRE(((uintptr_t)workspace & 255) == 0, "mvf_heat_grid: the workspace must be 256-byte aligned");
    const size_t need = heat_grid_ws_bytes(H, W);
    MVF_REQUIRE(workspace_bytes >= need, "mvf_heat_grid: workspace too small (%zu < %zu)", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int64_t total = H * W, nwg = heat_grid_nwg(H, W);
    char* base = (char*)workspace;
    HeatStatus* status = (HeatStatus*)base;
    double* buf[2] = {(double*)(base + 256), (double*)(base + 256) + total};
    double* part = buf[1] + total;
    uint8_t* fixed = (uint8_t*)(part + 2 * HEAT_T * nwg);
    const dim3 flat((unsigned)cdiv(total, HEAT_THREADS)), block(HEAT_THREADS);
    const dim3 grid((unsigned)cdiv(W, HEAT_TX), (unsigned)cdiv(H, HEAT_TY));
    // the dispatcher: HEAT_T sweeps per launch at every size - 2.4x (2048 x 2048) to 3.0x faster than one sweep per launch at every
    // raster measured, 8 x 8 to 2048 x 2048 (profiles/digitize.md); the one-sweep launch remains as steps == 1
    const int T = block_steps ? block_steps : HEAT_T;
    const long long budget = heat_budget(max_err, max_itr);
    hipLaunchKernelGGL(heat_status_init_kernel, dim3(1), block, 0, st, status);
    hipLaunchKernelGGL(heat_grid_prep_kernel, flat, block, 0, st, init, border, H, W, buf[0], fixed);
    MVF_LAUNCH_CHECK();
    HeatStatus hs;
    std::memset(&hs, 0, sizeof(hs));
    hs.err = 1.0, hs.hit = (1.0 > max_err) ? 1 : 0;  // (no sweep at all: the reference's starting err = 1)
    const double* result = buf[0];
    if (budget > 0) {
        long long launched = 0, batch = 0;
        hs.done = 0;
        while (!hs.done && launched < budget) {
            for (int p = 0; p < HEAT_POLL && launched < budget; ++p, ++batch) {
                const int steps = (int)std::min<long long>(T, budget - launched);
                hipLaunchKernelGGL(heat_grid_kernel, grid, block, 0, st, buf[batch & 1], buf[(batch + 1) & 1], fixed, mask, (int)H, (int)W,
                                   steps, status, part);
                hipLaunchKernelGGL(heat_finalize_kernel, dim3(1), block, 0, st, part, nwg, steps, max_err, max_itr, batch, status);
                launched += steps;
            }
            MVF_LAUNCH_CHECK();
            if (heat_read_status(st, status, &hs)) return 1;
        }
        MVF_REQUIRE(hs.done, "mvf_heat_grid: the sweep budget ran out without the stop flag (internal error)");
        const int steps_b = (int)std::min<long long>(T, budget - hs.batch * T);
        if (hs.stop_t + 1 < steps_b) {  // the stop fell inside its batch: that batch again, up to the stopping sweep
            hipLaunchKernelGGL(heat_grid_kernel, grid, block, 0, st, buf[hs.batch & 1], buf[(hs.batch + 1) & 1], fixed, mask, (int)H,
                               (int)W, (int)hs.stop_t + 1, (const HeatStatus*)nullptr, part);
        }
        result = buf[(hs.batch + 1) & 1];
    }
    hipLaunchKernelGGL(heat_grid_mask_kernel, flat, block, 0, st, result, mask, total, out);
    MVF_LAUNCH_CHECK();
    MVF_CHECK_HIP(hipStreamSynchronize(st));
    *sweeps = hs.sweeps, *err = hs.err, *hit_max_itr = (int)hs.hit;
    return 0;
}

extern "C" size_t mvf_heat_graph_workspace_bytes(int64_t n, int64_t nnz) {
    if (n < 1 || nnz < 0 || n >= ((int64_t)1 << 31) || nnz >= ((int64_t)1 << 40)) return 0;
    return heat_graph_ws_bytes(n, nnz);
}

extern "C" int mvf_heat_graph(const int64_t* indptr, const int32_t* indices, const double* values, const double* fixed_value, int64_t n,
                              double max_err, double max_itr, double* out, int64_t* sweeps, double* err, int* hit_max_itr,
                              void* workspace, size_t workspace_bytes, void* stream) {
    MVF_REQUIRE(n >= 1 && n < ((int64_t)1 << 31), "mvf_heat_graph: bad shape (n=%lld; at least 1 and below 2^31)", (long long)n);
    MVF_REQUIRE(indptr && fixed_value && out && sweeps && err && hit_max_itr, "mvf_heat_graph: null pointer");
    MVF_REQUIRE(indptr[0] == 0, "mvf_heat_graph: bad indptr (indptr[0] = %lld, not 0)", (long long)indptr[0]);
    for (int64_t j = 0; j < n; ++j)
        MVF_REQUIRE(indptr[j + 1] >= indptr[j], "mvf_heat_graph: bad indptr (it falls at column %lld)", (long long)j);
    const int64_t nnz = indptr[n];
    MVF_REQUIRE(nnz < ((int64_t)1 << 40), "mvf_heat_graph: bad shape (nnz=%lld)", (long long)nnz);
    MVF_REQUIRE(nnz == 0 || (indices && values), "mvf_heat_graph: null pointer (indices / values)");
    for (int64_t e = 0; e < nnz; ++e)
        MVF_REQUIRE(indices[e] >= 0 && indices[e] < n, "mvf_heat_graph: index out of range (indices[%lld] = %d, n = %lld)", (long long)e,
                    (int)indices[e], (long long)n);
    MVF_REQUIRE(workspace, "mvf_heat_graph: null pointer (workspace)");
    MVF_REQUIRE(((uintptr_t)workspace & 255) == 0, "mvf_heat_graph: the workspace must be 256-byte aligned");
    const size_t need = heat_graph_ws_bytes(n, nnz);
    MVF_REQUIRE(workspace_bytes >= need, "mvf_heat_graph: workspace too small (%zu < %zu)", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nwg = cdiv(n, HEAT_THREADS);
    char* base = (char*)workspace;
    HeatStatus* status = (HeatStatus*)base;
    double* buf[2] = {(double*)(base + 256), (double*)(base + 256) + n};
    double* fixedv = buf[1] + n;
    double* part = fixedv + n;
    double* d_vals = part + 2 * nwg;
    int64_t* d_indptr = (int64_t*)(d_vals + nnz);
    int32_t* d_indices = (int32_t*)(d_indptr + n + 1);
    const dim3 grid((unsigned)nwg), block(HEAT_THREADS);
    MVF_CHECK_HIP(hipMemcpyAsync(fixedv, fixed_value, (size_t)n * 8, hipMemcpyHostToDevice, st));
    MVF_CHECK_HIP(hipMemcpyAsync(d_indptr, indptr, (size_t)(n + 1) * 8, hipMemcpyHostToDevice, st));
    if (nnz) {
        MVF_CHECK_HIP(hipMemcpyAsync(d_vals, values, (size_t)nnz * 8, hipMemcpyHostToDevice, st));
        MVF_CHECK_HIP(hipMemcpyAsync(d_indices, indices, (size_t)nnz * 4, hipMemcpyHostToDevice, st));
    }
    MVF_CHECK_HIP(hipMemcpyAsync(buf[0], fixedv, (size_t)n * 8, hipMemcpyDeviceToDevice, st));  // the field starts as fixed_value
    hipLaunchKernelGGL(heat_status_init_kernel, dim3(1), block, 0, st, status);
    MVF_LAUNCH_CHECK();
    const long long budget = heat_budget(max_err, max_itr);
    HeatStatus hs;
    std::memset(&hs, 0, sizeof(hs));
    hs.err = 1.0, hs.hit = (1.0 > max_err) ? 1 : 0;  // (no sweep at all: the reference's starting err = 1)
    const double* result = buf[0];
    if (budget > 0) {
        long long batch = 0;
        hs.done = 0;
        while (!hs.done && batch < budget) {
            for (int p = 0; p < HEAT_POLL && batch < budget; ++p, ++batch) {
                hipLaunchKernelGGL(heat_graph_kernel, grid, block, 0, st, buf[batch & 1], buf[(batch + 1) & 1], d_indptr, d_indices, d_vals,
                                   fixedv, n, status, part);
                hipLaunchKernelGGL(heat_finalize_kernel, dim3(1), block, 0, st, part, nwg, 1, max_err, max_itr, batch, status);
            }
            MVF_LAUNCH_CHECK();
            if (heat_read_status(st, status, &hs)) return 1;
        }
        MVF_REQUIRE(hs.done, "mvf_heat_graph: the sweep budget ran out without the stop flag (internal error)");
        result = buf[(hs.batch + 1) & 1];
    }
    MVF_CHECK_HIP(hipMemcpyAsync(out, result, (size_t)n * 8, hipMemcpyDeviceToDevice, st));
    MVF_CHECK_HIP(hipStreamSynchronize(st));
    *sweeps = hs.sweeps, *err = hs.err, *hit_max_itr = (int)hs.hit;
    return 0;
}

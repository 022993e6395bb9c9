// Adaptive trajectory integration with SciPy's RK45 (morphopath as the reference runs it: spateo/tdr/morphometrics/
// morphofield/trajectory.py:61-110 hands the field to dynamo `fate`, which runs `solve_ivp(..., method="RK45",
// max_step=t_end/interpolation_num, dense_output=True, events=<field at rest>)` per cell).
//
// One lane per trajectory; state, stages and step control in float64 registers; control points and coefficients staged
// in LDS as integrate_kernel stages them (chunked when M exceeds the LDS cap).  The step is SciPy 1.15.3 line by line:
//   rk.py      RungeKutta._step_impl (min_step from nextafter, h clipped to [min_step, max_step] and to t_bound,
//              SAFETY / MIN_FACTOR / MAX_FACTOR, error exponent -1/5, factor <= 1 after a rejection), rk_step with the
//              Dormand-Prince tableau (FSAL), RkDenseOutput (Q = K^T P, x = (t - t_old) / h)
//   common.py  select_initial_step, norm = RMS over the field's own dimension d
//   ivp.py     find_active_events on the event values g = all(|v| < 1e-5) - 1 + 1e-12 between accepted steps,
//              solve_event_equation (brentq to xtol = rtol = 4 EPS: bisection of the step function to that width, the
//              root on the at-rest side as brentq returns it); the path ends at (root, sol(root))
// Step control, the event and the arc length act on the caller's WORLD coordinates y = q * scale + offset (q = the
// kernel's centred / normalised coordinate): the error scale atol + rtol max(|y_old|, |y_new|) needs absolute values.
//
// Sampling without a workspace.  uniform_time: one pass, targets k T / (n_out - 1), emitted on the dense output of the
// step that reaches them.  arc_length: the lane integrates twice with ONE instance of the step body (runtime pass
// variable, `#pragma unroll 1`): pass 0 yields the path length L, the end time and the status; pass 1 replays the same
// steps bit for bit and emits s_k = k L / (n_out - 1) as its step passes it (np.interp along the polyline of step
// points for the time, the step's dense output for the state).
//
// Barriers: when the control points do not fit in LDS, every field evaluation stages chunks between __syncthreads().
// Lanes take different numbers of steps, so in that case the step loop and the event bisection are block-uniform
// (`__syncthreads_or(active)`), finished lanes evaluate a harmless point and discard it.
#include "mvf_common.h"

namespace mvf {

struct Rk45Params {
    double scale[3], offset[3];  // y_world = q * scale + offset, per axis
    double t_bound, rtol, atol, max_step;
    int d, max_steps, sampling, n_out;
};

enum { RK45_RUNNING = 2 };

// Dormand-Prince 5(4) (rk.py class RK45), the constants as Python's true division rounds them
#define DP_A21 (1.0 / 5)
#define DP_A31 (3.0 / 40)
#define DP_A32 (9.0 / 40)
#define DP_A41 (44.0 / 45)
#define DP_A42 (-56.0 / 15)
#define DP_A43 (32.0 / 9)
#define DP_A51 (19372.0 / 6561)
#define DP_A52 (-25360.0 / 2187)
#define DP_A53 (64448.0 / 6561)
#define DP_A54 (-212.0 / 729)
#define DP_A61 (9017.0 / 3168)
#define DP_A62 (-355.0 / 33)
#define DP_A63 (46732.0 / 5247)
#define DP_A64 (49.0 / 176)
#define DP_A65 (-5103.0 / 18656)

__device__ __forceinline__ double dp_B(int k) {
    const double B[6] = {35.0 / 384, 0.0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
    return B[k];
}
__device__ __forceinline__ double dp_E(int k) {
    const double E[7] = {-71.0 / 57600, 0.0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};
    return E[k];
}
__device__ __forceinline__ double dp_P(int k, int j) {
    const double P[7][4] = {
        {1.0, -8048581381.0 / 2820520608, 8663915743.0 / 2820520608, -12715105075.0 / 11282082432},
        {0.0, 0.0, 0.0, 0.0},
        {0.0, 131558114200.0 / 32700410799, -68118460800.0 / 10900136933, 87487479700.0 / 32700410799},
        {0.0, -1754552775.0 / 470086768, 14199869525.0 / 1410260304, -10690763975.0 / 1880347072},
        {0.0, 127303824393.0 / 49829197408, -318862633887.0 / 49829197408, 701980252875.0 / 199316789632},
        {0.0, -282668133.0 / 205662961, 2019193451.0 / 616988883, -1453857185.0 / 822651844},
        {0.0, 40617522.0 / 29380423, -110615467.0 / 29380423, 69997945.0 / 29380423}};
    return P[k][j];
}

// Python's min / max (the first argument unless the second compares strictly smaller / larger) and NumPy's maximum
// (NaN propagates): the NaN behaviour of the controller is SciPy's
__device__ __forceinline__ double py_min(double a, double b) { return b < a ? b : a; }
__device__ __forceinline__ double py_max(double a, double b) { return b > a ? b : a; }
__device__ __forceinline__ double np_maximum(double a, double b) { return (a != a || b != b) ? a + b : (a > b ? a : b); }

template <typename T>
__global__ __launch_bounds__(256) void rk45_kernel(const T* __restrict__ x4, int64_t n, const T* __restrict__ ctrl4,
                                                   int64_t m, T s, EvalAffine af, const double* __restrict__ C, int chunk,
                                                   Rk45Params p, double* __restrict__ tout, double* __restrict__ traj,
                                                   int* __restrict__ stats) {
    using V4T = typename Vec4<T>::type;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_dyn[];
    V4T* sc = reinterpret_cast<V4T*>(smem_dyn);
    double4* sC = reinterpret_cast<double4*>(smem_dyn + (size_t)chunk * sizeof(V4T));
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = i < n;
    const int nchunks = (int)((m + chunk - 1) / chunk);
    const bool chunked = nchunks > 1;  // block-uniform
    const int d = p.d, n_out = p.n_out;
    const double dir = p.t_bound > 0.0 ? 1.0 : -1.0;

    auto stage = [&](int64_t m0) {
        const int mc = (int)min((int64_t)chunk, m - m0);
        for (int j = threadIdx.x; j < chunk; j += 256) {
            if (j < mc) {
                const V4T cv = reinterpret_cast<const V4T*>(ctrl4)[m0 + j];
                sc[j] = V4T{cv.x * s, cv.y * s, cv.z * s, 0};
                const double* cp = C + (m0 + j) * 3;
                sC[j] = double4{cp[0], cp[1], cp[2], 0.0};
            } else {
                sc[j] = V4T{0, 0, 0, 0};
                sC[j] = double4{0.0, 0.0, 0.0, 0.0};
            }
        }
    };
    // v_world(y_world): integrate_kernel's field on q = (y - offset) / scale, scaled back per axis; axes >= d are 0.
    // Chunked: every lane of the block must call it the same number of times (it holds barriers).
    auto field = [&](const double (&y)[3], double (&v)[3]) {
        const double q0 = (y[0] - p.offset[0]) / p.scale[0];
        const double q1 = (y[1] - p.offset[1]) / p.scale[1];
        const double q2 = (y[2] - p.offset[2]) / p.scale[2];
        const T px = (T)q0 * s, py = (T)q1 * s, pz = (T)q2 * s;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        for (int cidx = 0; cidx < nchunks; ++cidx) {
            if (chunked) {
                __syncthreads();
                stage((int64_t)cidx * chunk);
                __syncthreads();
            }
            const int mc = (int)min((int64_t)chunk, m - (int64_t)cidx * chunk);
#pragma unroll 4
            for (int j = 0; j < mc; ++j) {
                const V4T cv = sc[j];
                const double4 cc = sC[j];
                const double k = (double)kernel_value(px, py, pz, cv.x, cv.y, cv.z);
                a0 = fma(k, cc.x, a0), a1 = fma(k, cc.y, a1), a2 = fma(k, cc.z, a2);
            }
        }
        const double v0 = af.alpha[0] * a0 + af.A[0] * q0 + af.A[1] * q1 + af.A[2] * q2 + af.b[0];
        const double v1 = af.alpha[1] * a1 + af.A[3] * q0 + af.A[4] * q1 + af.A[5] * q2 + af.b[1];
        const double v2 = af.alpha[2] * a2 + af.A[6] * q0 + af.A[7] * q1 + af.A[8] * q2 + af.b[2];
        v[0] = v0 * p.scale[0];
        v[1] = d > 1 ? v1 * p.scale[1] : 0.0;
        v[2] = d > 2 ? v2 * p.scale[2] : 0.0;
    };
    // RMS norm over the d live components (common.py norm: np.linalg.norm(x) / x.size ** 0.5)
    auto rms = [&](double x0, double x1, double x2) {
        double ss = x0 * x0;
        if (d > 1) ss = ss + x1 * x1;
        if (d > 2) ss = ss + x2 * x2;
        return sqrt(ss) / sqrt((double)d);
    };
    // the event's sign: at rest <=> g = 1e-12 > 0 (g never vanishes, so "up" / "down" = a change of this flag)
    auto at_rest = [&](const double (&v)[3]) {
        bool r = fabs(v[0]) < 1e-5;
        if (d > 1) r = r && fabs(v[1]) < 1e-5;
        if (d > 2) r = r && fabs(v[2]) < 1e-5;
        return r;
    };

    if (!chunked) {
        stage(0);
        __syncthreads();
    }

    // start point in world coordinates; a non-finite row never enters the loop
    double y0[3] = {0.0, 0.0, 0.0};
    bool finite = false;
    if (live) {
        const V4T xv = reinterpret_cast<const V4T*>(x4)[i];
        const double xq[3] = {(double)xv.x, (double)xv.y, (double)xv.z};
        finite = true;
        for (int c = 0; c < 3; ++c) {
            const double w = c < d ? xq[c] * p.scale[c] + p.offset[c] : 0.0;
            finite = finite && isfinite(w);
            y0[c] = w;
        }
        if (!finite) y0[0] = y0[1] = y0[2] = 0.0;  // what this lane evaluates (and discards) in a chunked block
    }
    double* to = tout + (size_t)i * n_out;
    double* xo = traj + (size_t)i * n_out * 3;
    auto emit = [&](int k, double tq, double a, double b, double c) {
        to[k] = tq;
        double* o = xo + (size_t)k * 3;
        o[0] = a, o[1] = b, o[2] = c;
    };

    const bool arc = p.sampling == MVF_RK45_ARC_LENGTH;
    double L = 0.0, t_last = 0.0;  // pass 0's results
    int status = live ? (finite ? RK45_RUNNING : -3) : 0;
    int n_acc = 0, n_rej = 0, n_fev = 0;

#pragma unroll 1
    for (int pass = arc ? 0 : 1; pass < 2; ++pass) {
        const bool emitting = pass == 1 && live && finite;
        // targets of this pass: arc length s_k = k L / (n_out - 1) (np.linspace), or times k T / (n_out - 1) with
        // T = t_bound (uniform_time) or the path's end time (arc_length on a path of length 0: the oracle's linspace)
        const bool arc_targets = arc && L > 0.0;
        const double T_end = arc ? t_last : p.t_bound;
        const double sstep = L / (n_out - 1), tstep = T_end / (n_out - 1);
        auto s_target = [&](int k) { return k == n_out - 1 ? L : (double)k * sstep; };
        auto t_target = [&](int k) { return k == n_out - 1 ? T_end : (double)k * tstep; };

        double t = 0.0, y[3] = {y0[0], y0[1], y0[2]}, f[3];
        double s_acc = 0.0;  // arc length up to the current step point
        int k_next = 1;      // next sample to emit
        status = live ? (finite ? RK45_RUNNING : -3) : 0;
        bool active = status == RK45_RUNNING;
        n_acc = 0, n_rej = 0, n_fev = 0;
        if (emitting) emit(0, 0.0, y0[0], y0[1], y0[2]);

        // select_initial_step (common.py), f0 = fun(t0, y0) as RungeKutta.__init__ evaluates it
        field(y, f);
        double h_abs;
        {
            const double interval_length = fabs(p.t_bound);
            double sc3[3], f1[3], y1[3];
            for (int c = 0; c < 3; ++c) sc3[c] = p.atol + fabs(y[c]) * p.rtol;
            const double d0 = rms(y[0] / sc3[0], y[1] / sc3[1], y[2] / sc3[2]);
            const double d1 = rms(f[0] / sc3[0], f[1] / sc3[1], f[2] / sc3[2]);
            double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
            h0 = py_min(h0, interval_length);
            for (int c = 0; c < 3; ++c) y1[c] = y[c] + h0 * dir * f[c];
            field(y1, f1);
            const double d2 =
                rms((f1[0] - f[0]) / sc3[0], (f1[1] - f[1]) / sc3[1], (f1[2] - f[2]) / sc3[2]) / h0;
            const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? py_max(1e-6, h0 * 1e-3)
                                                           : pow(0.01 / py_max(d1, d2), 1.0 / (4 + 1));
            h_abs = py_min(py_min(py_min(100 * h0, h1), interval_length), p.max_step);
        }
        if (active) n_fev = 2;
        bool rest = at_rest(f);  // g(t0, y0)
        bool new_step = true, rejected = false;
        double min_step = 0.0;

        while (chunked ? __syncthreads_or(active) : active) {
            // ---- one attempt of RungeKutta._step_impl ----
            if (active && new_step) {
                min_step = 10 * fabs(nextafter(t, dir * INFINITY) - t);
                if (h_abs > p.max_step) h_abs = p.max_step;
                else if (h_abs < min_step) h_abs = min_step;
                new_step = false, rejected = false;
            }
            if (active && h_abs < min_step) status = -1, active = false;                // TOO_SMALL_STEP
            if (active && n_acc + n_rej >= p.max_steps) status = -2, active = false;   // this library's cap
            double h = h_abs * dir, t_new = t + h;
            if (dir * (t_new - p.t_bound) > 0) t_new = p.t_bound;
            h = t_new - t;
            if (!active) h = 0.0;  // a finished lane evaluates its own point (chunked blocks only)
            double K[7][3], yt[3];
            for (int c = 0; c < 3; ++c) K[0][c] = f[c];
            for (int c = 0; c < 3; ++c) yt[c] = y[c] + (K[0][c] * DP_A21) * h;
            field(yt, K[1]);
            for (int c = 0; c < 3; ++c) yt[c] = y[c] + (K[0][c] * DP_A31 + K[1][c] * DP_A32) * h;
            field(yt, K[2]);
            for (int c = 0; c < 3; ++c) yt[c] = y[c] + (K[0][c] * DP_A41 + K[1][c] * DP_A42 + K[2][c] * DP_A43) * h;
            field(yt, K[3]);
            for (int c = 0; c < 3; ++c)
                yt[c] = y[c] + (K[0][c] * DP_A51 + K[1][c] * DP_A52 + K[2][c] * DP_A53 + K[3][c] * DP_A54) * h;
            field(yt, K[4]);
            for (int c = 0; c < 3; ++c)
                yt[c] = y[c] + (K[0][c] * DP_A61 + K[1][c] * DP_A62 + K[2][c] * DP_A63 + K[3][c] * DP_A64 +
                                K[4][c] * DP_A65) * h;
            field(yt, K[5]);
            double y_new[3];
            for (int c = 0; c < 3; ++c) {
                double acc = 0.0;
                for (int k = 0; k < 6; ++k) acc = acc + K[k][c] * dp_B(k);
                y_new[c] = y[c] + h * acc;
            }
            field(y_new, K[6]);  // f_new (FSAL)
            bool accepted = false;
            if (active) {
                n_fev += 6;
                h_abs = fabs(h);
                double e[3];
                for (int c = 0; c < 3; ++c) {
                    double acc = 0.0;
                    for (int k = 0; k < 7; ++k) acc = acc + K[k][c] * dp_E(k);
                    const double sc = p.atol + np_maximum(fabs(y[c]), fabs(y_new[c])) * p.rtol;
                    e[c] = (acc * h) / sc;
                }
                const double error_norm = rms(e[0], e[1], e[2]);
                if (error_norm < 1) {
                    double factor = error_norm == 0 ? 10.0 : py_min(10.0, 0.9 * pow(error_norm, -1.0 / (4 + 1)));
                    if (rejected) factor = py_min(1.0, factor);
                    h_abs *= factor;
                    accepted = true;
                } else {
                    h_abs *= py_max(0.2, 0.9 * pow(error_norm, -1.0 / (4 + 1)));
                    rejected = true;
                    ++n_rej;
                }
            }
            // dense output of this step (RkDenseOutput: Q = K^T P, sol(tq) = y_old + h Q [x, x^2, x^3, x^4])
            double Q[3][4];
            for (int c = 0; c < 3; ++c)
                for (int j = 0; j < 4; ++j) {
                    double acc = 0.0;
                    for (int k = 0; k < 7; ++k) acc = acc + K[k][c] * dp_P(k, j);
                    Q[c][j] = acc;
                }
            auto sol = [&](double tq, double (&out)[3]) {
                const double x = (tq - t) / h;
                const double p1 = x, p2 = p1 * x, p3 = p2 * x, p4 = p3 * x;
                for (int c = 0; c < 3; ++c) out[c] = h * (Q[c][0] * p1 + Q[c][1] * p2 + Q[c][2] * p3 + Q[c][3] * p4) + y[c];
            };
            // ---- events between accepted steps (ivp.py find_active_events / solve_event_equation) ----
            const bool rest_new = at_rest(K[6]);
            bool fire = accepted && rest_new != rest;
            double a = t, b = t_new;  // bracket: rest(a) == rest, rest(b) == rest_new
            {
                bool bis = fire;
                int it = 0;
                auto converged = [&]() {
                    const double xr = rest ? a : b;  // brentq's best estimate: the side where |g| = 1e-12
                    const double tol = 4 * 2.220446049250313e-16 + 4 * 2.220446049250313e-16 * fabs(xr);
                    return !(fabs(b - a) >= tol);
                };
                if (bis && converged()) bis = false;
                while (chunked ? __syncthreads_or(bis) : bis) {
                    const double mid = bis ? a + (b - a) * 0.5 : t;
                    double ym[3], vm[3];
                    sol(mid, ym);
                    field(ym, vm);
                    if (bis) {
                        ++n_fev;
                        if (mid == a || mid == b) {
                            bis = false;  // the bracket cannot be split further
                        } else {
                            if (at_rest(vm) == rest) a = mid;
                            else b = mid;
                            if (converged() || ++it >= 100) bis = false;  // (brentq's maxiter)
                        }
                    }
                }
            }
            if (accepted) {
                // the new path point: the step's end, or (root, sol(root)) on a terminal event
                double t_pt = t_new, y_pt[3] = {y_new[0], y_new[1], y_new[2]};
                if (fire) {
                    t_pt = rest ? a : b;
                    sol(t_pt, y_pt);
                    status = 1;
                } else if (dir * (t_new - p.t_bound) >= 0) {
                    status = 0;
                }
                const bool done = status != RK45_RUNNING;
                const double dx = y_pt[0] - y[0], dy = y_pt[1] - y[1], dz = y_pt[2] - y[2];
                double ss = dx * dx;
                if (d > 1) ss = ss + dy * dy;
                if (d > 2) ss = ss + dz * dz;
                const double s_new = s_acc + sqrt(ss);
                if (emitting) {
                    double yq[3];
                    if (arc_targets) {  // np.interp(s_k, s, t) on this segment, the state on this step's dense output
                        for (; k_next < n_out; ++k_next) {
                            const double sq = s_target(k_next);
                            if (!(sq < s_new) && !done) break;
                            double tq = t_pt;
                            if (sq < s_new)
                                tq = sq == s_acc ? t : (t_pt - t) / (s_new - s_acc) * (sq - s_acc) + t;
                            sol(tq, yq);
                            emit(k_next, tq, yq[0], yq[1], yq[2]);
                        }
                    } else {  // time targets up to this point; after the path's end, its end state
                        for (; k_next < n_out; ++k_next) {
                            const double tq = t_target(k_next);
                            const bool inside = dir * (tq - t_pt) <= 0;
                            if (!inside && !done) break;
                            if (inside) sol(tq, yq);
                            else yq[0] = y_pt[0], yq[1] = y_pt[1], yq[2] = y_pt[2];
                            emit(k_next, tq, yq[0], yq[1], yq[2]);
                        }
                    }
                }
                t = t_pt, s_acc = s_new;
                for (int c = 0; c < 3; ++c) y[c] = y_pt[c], f[c] = K[6][c];
                rest = rest_new;
                ++n_acc;
                new_step = true;
                if (done) active = false;
            }
        }
        // a path that ended without reaching its end (status -1 / -2): the remaining samples hold its last point
        if (emitting && (status == -1 || status == -2))
            for (; k_next < n_out; ++k_next) emit(k_next, arc_targets ? t : t_target(k_next), y[0], y[1], y[2]);
        if (pass == 0) L = s_acc, t_last = t;
    }
    if (!live) return;
    if (!finite) {
        const double nan = __builtin_nan("");
        for (int k = 0; k < n_out; ++k) emit(k, nan, nan, nan, nan);
    }
    int* so = stats + (size_t)i * 4;
    so[0] = n_acc, so[1] = n_rej, so[2] = n_fev, so[3] = status;
}

}  // namespace mvf

using namespace mvf;

extern "C" int mvf_integrate_rk45(const void* x4, int64_t n, const void* ctrl4, int64_t m, double beta, const double* C,
                                  const double* affine, int d, const double* world, double t_bound, double rtol,
                                  double atol, double max_step, int max_steps, int sampling, int n_out, double* t,
                                  double* traj, int* stats, mvf_dtype dtype, void* stream) {
    MVF_REQUIRE(n >= 0 && m >= 0, "mvf_integrate_rk45: bad shape");
    MVF_REQUIRE(d >= 1 && d <= 3, "mvf_integrate_rk45: d must be 1, 2 or 3 (got %d)", d);
    MVF_REQUIRE(n_out >= 2, "mvf_integrate_rk45: n_out must be >= 2 (got %d)", n_out);
    MVF_REQUIRE(beta > 0.0 && std::isfinite(beta), "mvf_integrate_rk45: beta must be finite and > 0");
    MVF_REQUIRE(std::isfinite(t_bound) && t_bound != 0.0, "mvf_integrate_rk45: t_bound must be finite and non-zero");
    MVF_REQUIRE(rtol > 0.0 && std::isfinite(rtol), "mvf_integrate_rk45: rtol must be finite and > 0");
    MVF_REQUIRE(atol > 0.0 && std::isfinite(atol), "mvf_integrate_rk45: atol must be finite and > 0");
    MVF_REQUIRE(max_step > 0.0 && !std::isnan(max_step), "mvf_integrate_rk45: max_step must be > 0");
    MVF_REQUIRE(max_steps >= 1, "mvf_integrate_rk45: max_steps must be >= 1");
    MVF_REQUIRE(sampling == MVF_RK45_UNIFORM_TIME || sampling == MVF_RK45_ARC_LENGTH,
                "mvf_integrate_rk45: bad sampling code %d", sampling);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_F64, "mvf_integrate_rk45: bad dtype %d", (int)dtype);
    MVF_REQUIRE(world, "mvf_integrate_rk45: null world map");
    Rk45Params p;
    for (int c = 0; c < 3; ++c) {
        p.scale[c] = world[c], p.offset[c] = world[3 + c];
        MVF_REQUIRE(std::isfinite(p.scale[c]) && p.scale[c] != 0.0 && std::isfinite(p.offset[c]),
                    "mvf_integrate_rk45: world scale must be finite and non-zero, offset finite");
    }
    if (n == 0) return 0;
    MVF_REQUIRE(x4 && t && traj && stats && (m == 0 || (ctrl4 && C)), "mvf_integrate_rk45: null pointer");
    p.t_bound = t_bound, p.rtol = rtol, p.atol = atol, p.max_step = max_step;
    p.d = d, p.max_steps = max_steps, p.sampling = sampling, p.n_out = n_out;
    const EvalAffine af = eval_affine_from_host(affine);
    hipStream_t st = (hipStream_t)stream;
    const double s = std::sqrt(beta * LOG2E);
    const size_t per = (dtype == MVF_F32 ? 16 : 32) + 32;  // LDS per staged control point, as mvf_integrate
    const int cap = (int)((144 * 1024) / per);
    const int chunk = (int)std::max<int64_t>(1, std::min<int64_t>(m, cap));
    const size_t lds = (size_t)chunk * per;
    dim3 grid((unsigned)cdiv(n, 256));
    if (dtype == MVF_F32) {
        MVF_CHECK_HIP(hipFuncSetAttribute((const void*)rk45_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds));
        hipLaunchKernelGGL(rk45_kernel<float>, grid, dim3(256), lds, st, (const float*)x4, n, (const float*)ctrl4, m,
                           (float)s, af, C, chunk, p, t, traj, stats);
    } else {
        MVF_CHECK_HIP(hipFuncSetAttribute((const void*)rk45_kernel<double>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                          (int)lds));
        hipLaunchKernelGGL(rk45_kernel<double>, grid, dim3(256), lds, st, (const double*)x4, n, (const double*)ctrl4, m,
                           s, af, C, chunk, p, t, traj, stats);
    }
    MVF_LAUNCH_CHECK();
    return 0;
}

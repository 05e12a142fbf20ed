// Flatfield ESTIMATE on the device: replaces
//     basicpy.BaSiC(get_darkfield=False, smoothness_flatfield=s).fit(images).flatfield
// of the reference's get_flatfields (stitcher.py:365-419; the call is :374-377).
//
// PARITY UNPINNED: basicpy (and its jax dependency) is an un-pinned third-party package that is absent offline; no
// output of it exists to compare with.  This is the PUBLISHED algorithm -- BaSiC, Peng et al., Nat. Commun. 8:14836
// (2017): I_i(x) = b_i S(x) + R_i(x), S sparse in the DCT domain, R sparse in the image domain, solved by LADMAP
// inside an iteratively re-weighted L1 loop -- in the configuration the reference asks for (no darkfield) with
// basicpy's documented defaults, and its definition is oracle/basic_oracle.py (tests compare the two; they also
// recover a planted gain).  The DIVIDE by the gains is on the hot path (fuse.hip); this estimate runs once per
// channel before it and is not: <= 80 images are resampled to 128 x 128 and a few hundred iterations of
// element-wise work + four 128^3 matrix products follow -- microseconds of HBM time, launch-latency bound.
//
// Kernels (float32 like basicpy; sums that decide convergence are accumulated in float64):
//   resample_rows / resample_cols   separable triangle-kernel resize (anti-aliased when shrinking), banded weights
//   median_kernel                   S0 = per-pixel median over the images
//   gram_kernel                     A A^T of the [n x 16384] stack (spectral norm on the host: n <= 80)
//   s_linear_kernel                 S + sum_i b_i (I_i - b_i S - R_i + Y_i / mu) / eta
//   s_dct_shrink_kernel             S <- C^T shrink(C S C^T, smoothness / (eta mu)) C   (one workgroup, LDS)
//   residual_kernel                 R_i <- shrink(I_i - b_i S + Y_i / mu, W_i / mu);  b_i <- max(<S, I_i - R_i + Y_i/mu> / <S,S>, 0)
//   multiplier_kernel               Y_i += mu (I_i - R_i - b_i S)
//   step_kernel                     change / residual norms -> mu update, convergence flag
//   reweight_kernel(s)              S /= mean S, b *= mean S, W = 1 / (|R / (b S + eps)| + eps) normalised to mean 1
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"

using namespace sq;

namespace {

constexpr int WS = 128;             // working size (basicpy default)
constexpr int NPIX = WS * WS;
constexpr int MAX_IMAGES = 80;      // stitcher.py:381-395: <= 32 per timepoint until MORE than 48 are held -> at most 48 + 32
constexpr float EPSILON = 0.1f;
constexpr double RHO = 1.5, MU_COEF = 12.5, MAX_MU_COEF = 1e7, OPT_TOL = 1e-3, REWEIGHT_TOL = 1e-2;
constexpr int MAX_ITER = 500, MAX_REWEIGHT = 10;

struct Scalars {          // device-side state of one LADMAP solve
    double ds2, dr2, db2, fit2, s2;     // squared norms accumulated by the kernels of one iteration
    double image_norm;
    float mu, max_mu, eta, thr_s;       // thr_s = smoothness / (eta mu)
    float smoothness;
    int converged, iterations;
    double mean_s, mean_w, mad_num, mad_den;   // reweighting
};

struct Band {             // banded resampling weights of one axis: out[o] = sum_k w[o][k] in[start[o] + k]
    const int *start;
    const float *w;
    int width;
};

__device__ __forceinline__ float shrinkf(float x, float t) {
    const float a = fabsf(x) - t;
    return a > 0.0f ? copysignf(a, x) : 0.0f;
}

__device__ __forceinline__ double block_sum(double v, double *red) {   // 256 threads
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
    return t;
}

// tmp[i][o][x] = sum_k wy[o][k] img_i[y0[o] + k][x]
template <typename T>
__global__ __launch_bounds__(256) void resample_rows_kernel(const void *const *ptrs, const void *base, int64_t stride, int pitch,
                                                            int w_in, Band by, float *tmp) {
    const int i = blockIdx.y, o = blockIdx.x;
    const T *img = ptrs ? static_cast<const T *>(ptrs[i]) : static_cast<const T *>(base) + i * stride;
    const int y0 = by.start[o];
    for (int x = threadIdx.x; x < w_in; x += blockDim.x) {
        float acc = 0.0f;
        for (int k = 0; k < by.width; ++k) {
            const float wk = by.w[o * by.width + k];
            if (wk != 0.0f) acc = fmaf(wk, (float)img[(int64_t)(y0 + k) * pitch + x], acc);
        }
        tmp[((int64_t)i * WS + o) * w_in + x] = acc;
    }
}
// out[i][o][p] = sum_k wx[p][k] tmp[i][o][x0[p] + k]
__global__ __launch_bounds__(128) void resample_cols_kernel(const float *tmp, int w_in, Band bx, float *out) {
    const int i = blockIdx.y, o = blockIdx.x, p = threadIdx.x;
    const float *row = tmp + ((int64_t)i * WS + o) * w_in;
    const int x0 = bx.start[p];
    float acc = 0.0f;
    for (int k = 0; k < bx.width; ++k) {
        const float wk = bx.w[p * bx.width + k];
        if (wk != 0.0f) acc = fmaf(wk, row[x0 + k], acc);
    }
    out[((int64_t)i * WS + o) * WS + p] = acc;
}
// the way back: flat[y][x] = sum_o sum_p wy[y][.] wx[x][.] S[o][p]  (two taps per axis when enlarging)
__global__ __launch_bounds__(256) void resample_up_kernel(const float *s, int h_out, int w_out, Band by, Band bx, float *flat) {
    const int y = blockIdx.x;
    const int o0 = by.start[y];
    for (int x = threadIdx.x; x < w_out; x += blockDim.x) {
        const int p0 = bx.start[x];
        float acc = 0.0f;
        for (int a = 0; a < by.width; ++a) {
            const float wa = by.w[y * by.width + a];
            if (wa == 0.0f) continue;
            float row = 0.0f;
            for (int c = 0; c < bx.width; ++c) {
                const float wc = bx.w[x * bx.width + c];
                if (wc != 0.0f) row = fmaf(wc, s[(o0 + a) * WS + p0 + c], row);
            }
            acc = fmaf(wa, row, acc);
        }
        flat[(int64_t)y * w_out + x] = acc;
    }
}

__global__ __launch_bounds__(256) void median_kernel(const float *im, int n, float *s) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= NPIX) return;
    float v[MAX_IMAGES];
    for (int i = 0; i < n; ++i) {   // insertion sort
        const float x = im[(int64_t)i * NPIX + p];
        int j = i;
        while (j > 0 && v[j - 1] > x) {
            v[j] = v[j - 1];
            --j;
        }
        v[j] = x;
    }
    s[p] = (n & 1) ? v[n / 2] : 0.5f * (v[n / 2 - 1] + v[n / 2]);   // numpy.median
}

__global__ __launch_bounds__(256) void gram_kernel(const float *im, int n, double *gram) {
    __shared__ double red[4];
    const int i = blockIdx.x, j = blockIdx.y;
    if (j > i) return;
    double acc = 0.0;
    for (int p = threadIdx.x; p < NPIX; p += blockDim.x) acc += (double)im[(int64_t)i * NPIX + p] * (double)im[(int64_t)j * NPIX + p];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) gram[i * n + j] = gram[j * n + i] = acc;
}

__global__ void solve_init_kernel(Scalars *sc, float *b, int n, float *r, float *y, float init_mu) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (int64_t e = gid; e < (int64_t)n * NPIX; e += (int64_t)gridDim.x * blockDim.x) r[e] = y[e] = 0.0f;
    if (gid < n) b[gid] = 1.0f;
    if (gid == 0) {
        sc->mu = init_mu;
        sc->max_mu = (float)((double)init_mu * MAX_MU_COEF);
        sc->converged = 0;
        sc->iterations = 0;
        sc->ds2 = sc->dr2 = sc->db2 = sc->fit2 = sc->s2 = 0.0;
    }
}

// eta = sum b^2 * 1.02 + 0.01 (float32 like the definition), threshold for the DCT shrink; zero the accumulators
__global__ void iter_begin_kernel(Scalars *sc, const float *b, int n) {
    if (sc->converged) return;
    float sb = 0.0f;
    for (int i = 0; i < n; ++i) sb += b[i] * b[i];
    sc->eta = sb * 1.02f + 0.01f;
    sc->thr_s = sc->smoothness / (sc->eta * sc->mu);
    sc->ds2 = sc->dr2 = sc->db2 = sc->fit2 = sc->s2 = 0.0;
}

__global__ __launch_bounds__(256) void s_linear_kernel(const Scalars *sc, const float *im, const float *r, const float *y,
                                                       const float *b, int n, const float *s, float *s_lin) {
    if (sc->converged) return;
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= NPIX) return;
    const float mu = sc->mu, eta = sc->eta, sp = s[p];
    float acc = 0.0f;
    for (int i = 0; i < n; ++i) {
        const int64_t e = (int64_t)i * NPIX + p;
        acc += b[i] * (im[e] - b[i] * sp - r[e] + y[e] / mu);
    }
    s_lin[p] = sp + acc / eta;
}

// One workgroup: X <- C X C^T, shrink, X <- C^T X C.  X and C live in LDS (64 + 64.5 KB); every thread owns 16 outputs
// of each of the four products and sums over k in ascending order.  The rows of C are CS = 129 floats apart: the second
// product reads C[c][k] with c running over the lanes, which at a stride of 128 floats puts all 32 lanes of a half-wave
// on one bank (this kernel is most of a fit's time); the sums and their order are untouched.
constexpr int CS = WS + 1;
constexpr int DCT_LDS_BYTES = (NPIX + WS * CS) * 4;
__global__ __launch_bounds__(1024) void s_dct_shrink_kernel(Scalars *sc, const float *cmat, const float *s_lin, float *s) {
    if (sc->converged) return;
    extern __shared__ float lds[];
    float *X = lds, *C = lds + NPIX;
    __shared__ double red[16];
    const int tid = threadIdx.x;
    for (int e = tid; e < NPIX; e += 1024) {
        X[e] = s_lin[e];
        C[(e >> 7) * CS + (e & 127)] = cmat[e];
    }
    __syncthreads();
    float out[16];
    auto product = [&](auto &&left, auto &&right) {   // X <- sum_k left(r, k) * right(k, c), r = row, c = column
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int e = tid + 1024 * q, rr = e >> 7, cc = e & 127;
            float acc = 0.0f;
            for (int k = 0; k < WS; ++k) acc = fmaf(left(rr, k), right(k, cc), acc);
            out[q] = acc;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) X[tid + 1024 * q] = out[q];
        __syncthreads();
    };
    product([&](int r_, int k) { return C[r_ * CS + k]; }, [&](int k, int c_) { return X[k * WS + c_]; });    // C X
    product([&](int r_, int k) { return X[r_ * WS + k]; }, [&](int k, int c_) { return C[c_ * CS + k]; });    // (C X) C^T
    const float thr = sc->thr_s;
    for (int e = tid; e < NPIX; e += 1024) X[e] = shrinkf(X[e], thr);
    __syncthreads();
    product([&](int r_, int k) { return C[k * CS + r_]; }, [&](int k, int c_) { return X[k * WS + c_]; });    // C^T X
    product([&](int r_, int k) { return X[r_ * WS + k]; }, [&](int k, int c_) { return C[k * CS + c_]; });    // (C^T X) C
    double ds2 = 0.0, s2 = 0.0;
    for (int e = tid; e < NPIX; e += 1024) {
        const float nv = X[e], ov = s[e];
        ds2 += (double)(nv - ov) * (double)(nv - ov);
        s2 += (double)nv * (double)nv;
        s[e] = nv;
    }
    for (int off = 32; off > 0; off >>= 1) {
        ds2 += __shfl_xor(ds2, off);
        s2 += __shfl_xor(s2, off);
    }
    if ((tid & 63) == 0) red[tid >> 6] = ds2;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += red[w];
        sc->ds2 = t;
    }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = s2;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < 16; ++w) t += red[w];
        sc->s2 = t;
    }
}

// one block per image
__global__ __launch_bounds__(256) void residual_kernel(Scalars *sc, const float *im, float *r, const float *y, const float *wt,
                                                       const float *s, float *b) {
    if (sc->converged) return;
    __shared__ double red[4];
    const int i = blockIdx.x;
    const float mu = sc->mu, bi = b[i];
    double dr2 = 0.0, num = 0.0;
    for (int p = threadIdx.x; p < NPIX; p += blockDim.x) {
        const int64_t e = (int64_t)i * NPIX + p;
        const float yv = y[e] / mu;
        const float rn = shrinkf(im[e] - bi * s[p] + yv, wt[e] / mu);
        const float d = rn - r[e];
        dr2 += (double)d * (double)d;
        r[e] = rn;
        num += (double)(s[p] * (im[e] - rn + yv));
    }
    dr2 = block_sum(dr2, red);
    num = block_sum(num, red);
    if (threadIdx.x == 0) {
        atomicAdd(&sc->dr2, dr2);
        const float bn = fmaxf((float)(num / sc->s2), 0.0f);
        const double db = (double)bn - (double)bi;
        atomicAdd(&sc->db2, db * db);
        b[i] = bn;
    }
}

__global__ __launch_bounds__(256) void multiplier_kernel(Scalars *sc, const float *im, const float *r, float *y, const float *s,
                                                         const float *b) {
    if (sc->converged) return;
    __shared__ double red[4];
    const int i = blockIdx.x;
    const float mu = sc->mu, bi = b[i];
    double f2 = 0.0;
    for (int p = threadIdx.x; p < NPIX; p += blockDim.x) {
        const int64_t e = (int64_t)i * NPIX + p;
        const float fit = im[e] - r[e] - bi * s[p];
        y[e] += mu * fit;
        f2 += (double)fit * (double)fit;
    }
    f2 = block_sum(f2, red);
    if (threadIdx.x == 0) atomicAdd(&sc->fit2, f2);
}

__global__ void step_kernel(Scalars *sc) {
    if (sc->converged) return;
    sc->iterations += 1;
    const double change = fmax(fmax(sqrt((double)sc->eta) * sqrt(sc->ds2), sqrt(sc->dr2)), sqrt(sc->s2) * sqrt(sc->db2)) / sc->image_norm;
    const double residual = sqrt(sc->fit2) / sc->image_norm;
    if ((double)sc->mu * change < 1e-2 * OPT_TOL * 10) sc->mu = (float)fmin((double)sc->mu * RHO, (double)sc->max_mu);
    if ((residual <= OPT_TOL && change <= OPT_TOL) || sc->iterations >= MAX_ITER) sc->converged = 1;
}

// re-weighting: S /= mean(S), b *= mean(S); W = 1 / (|R / (b S + eps)| + eps), then W /= mean(W); mad vs the last S
__global__ __launch_bounds__(1024) void reweight_s_kernel(Scalars *sc, float *s, float *b, int n, const float *last, int have_last) {
    __shared__ double red[16];
    const int tid = threadIdx.x;
    float acc = 0.0f;      // float32 mean like numpy's (pairwise there, strided here: within the test tolerance)
    for (int e = tid; e < NPIX; e += 1024) acc += s[e];
    double t = acc;
    for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off);
    if ((tid & 63) == 0) red[tid >> 6] = t;
    __syncthreads();
    double total = 0.0;
    for (int w = 0; w < 16; ++w) total += red[w];
    const float mean_s = (float)(total / NPIX);
    __syncthreads();
    double num = 0.0, den = 0.0;
    for (int e = tid; e < NPIX; e += 1024) {
        const float v = s[e] / mean_s;
        s[e] = v;
        if (have_last) {
            num += fabs((double)v - (double)last[e]);
            den += fabs((double)last[e]);
        }
    }
    if (tid < n) b[tid] *= mean_s;
    for (int off = 32; off > 0; off >>= 1) {
        num += __shfl_xor(num, off);
        den += __shfl_xor(den, off);
    }
    if ((tid & 63) == 0) red[tid >> 6] = num;
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
        for (int w = 0; w < 16; ++w) a += red[w];
        sc->mad_num = a;
        sc->mean_s = mean_s;
        sc->mean_w = 0.0;
    }
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = den;
    __syncthreads();
    if (tid == 0) {
        double a = 0.0;
        for (int w = 0; w < 16; ++w) a += red[w];
        sc->mad_den = a;
    }
}
__global__ __launch_bounds__(256) void reweight_w_kernel(Scalars *sc, const float *r, const float *s, const float *b, float *wt) {
    __shared__ double red[4];
    const int i = blockIdx.x;
    double sum = 0.0;
    for (int p = threadIdx.x; p < NPIX; p += blockDim.x) {
        const int64_t e = (int64_t)i * NPIX + p;
        const float w = 1.0f / (fabsf(r[e] / (b[i] * s[p] + EPSILON)) + EPSILON);
        wt[e] = w;
        sum += w;
    }
    sum = block_sum(sum, red);
    if (threadIdx.x == 0) atomicAdd(&sc->mean_w, sum);
}
__global__ void reweight_norm_kernel(const Scalars *sc, float *wt, int n) {
    const float mean_w = (float)(sc->mean_w / ((double)n * NPIX));
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < (int64_t)n * NPIX; e += (int64_t)gridDim.x * blockDim.x)
        wt[e] /= mean_w;
}
__global__ void fill_kernel(float *p, int64_t n, float v) {
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) p[e] = v;
}

// ---- host side -------------------------------------------------------------------------------------------------
// jax.image.resize(method='linear') per axis: triangle kernel around half-pixel centres, widened by the scale when
// shrinking, rows normalised to sum 1 (oracle/basic_oracle.py resize_matrix); float64 -> float32 like there
struct HostBand {
    std::vector<int> start;
    std::vector<float> w;
    int width = 0;
};
HostBand make_band(int n_out, int n_in) {
    const double scale = (double)n_in / n_out, width = std::max(scale, 1.0);
    HostBand B;
    B.width = std::min(n_in, (int)std::ceil(2 * width) + 2);
    B.start.resize(n_out);
    B.w.assign((size_t)n_out * B.width, 0.0f);
    std::vector<double> row(n_in);
    for (int o = 0; o < n_out; ++o) {
        const double c = (o + 0.5) * scale;
        double sum = 0.0;
        int lo = n_in, hi = -1;
        for (int j = 0; j < n_in; ++j) {
            const double d = std::fabs(c - (j + 0.5)) / width;
            row[j] = d < 1.0 ? 1.0 - d : 0.0;
            if (row[j] > 0.0) {
                sum += row[j];
                lo = std::min(lo, j);
                hi = j;
            }
        }
        lo = std::min(lo, n_in - B.width);
        lo = std::max(lo, 0);
        B.start[o] = lo;
        for (int k = 0; k < B.width && lo + k < n_in; ++k) B.w[(size_t)o * B.width + k] = (float)(row[lo + k] / sum);
        (void)hi;
    }
    return B;
}

// largest eigenvalue of a symmetric positive semi-definite n x n matrix (power iteration, float64)
double largest_eigenvalue(const std::vector<double> &g, int n) {
    std::vector<double> v(n, 1.0), u(n);
    double lam = 0.0;
    for (int it = 0; it < 1000; ++it) {
        double norm = 0.0;
        for (int i = 0; i < n; ++i) {
            double a = 0.0;
            for (int j = 0; j < n; ++j) a += g[(size_t)i * n + j] * v[j];
            u[i] = a;
            norm += a * a;
        }
        norm = std::sqrt(norm);
        if (norm == 0.0) return 0.0;
        for (int i = 0; i < n; ++i) v[i] = u[i] / norm;
        if (std::fabs(norm - lam) <= 1e-14 * norm) return norm;
        lam = norm;
    }
    return lam;
}

struct WsLayout {
    int64_t im, r, y, wt, tmp, s, s_lin, last, b, gram, cmat, scalars, by_start, by_w, bx_start, bx_w, uy_start, uy_w, ux_start, ux_w, total;
};
int64_t up16(int64_t v) { return (v + 255) & ~int64_t(255); }
WsLayout ws_layout(int n, int h, int w, int wy, int wx, int uy, int ux) {
    WsLayout L{};
    int64_t off = 0;
    auto take = [&](int64_t bytes) {
        const int64_t at = off;
        off += up16(bytes);
        return at;
    };
    const int64_t stack = (int64_t)n * NPIX * 4;
    L.im = take(stack);
    L.r = take(stack);
    L.y = take(stack);
    L.wt = take(stack);
    L.tmp = take((int64_t)n * WS * w * 4);
    L.s = take(NPIX * 4);
    L.s_lin = take(NPIX * 4);
    L.last = take(NPIX * 4);
    L.b = take(MAX_IMAGES * 4);
    L.gram = take((int64_t)n * n * 8);
    L.cmat = take(NPIX * 4);
    L.scalars = take(sizeof(Scalars));
    L.by_start = take(WS * 4);
    L.by_w = take((int64_t)WS * wy * 4);
    L.bx_start = take(WS * 4);
    L.bx_w = take((int64_t)WS * wx * 4);
    L.uy_start = take((int64_t)h * 4);
    L.uy_w = take((int64_t)h * uy * 4);
    L.ux_start = take((int64_t)w * 4);
    L.ux_w = take((int64_t)w * ux * 4);
    L.total = off;
    return L;
}

}  // namespace

extern "C" int64_t sq_basic_workspace_bytes(int32_t n_images, int32_t tile_h, int32_t tile_w) {
    if (n_images < 1 || n_images > MAX_IMAGES || tile_h < 1 || tile_w < 1)
        return fail(SQ_ERR_INVALID, "sq_basic_workspace_bytes: %d images of %dx%d (1..%d images)", n_images, tile_h, tile_w, MAX_IMAGES);
    const HostBand by = make_band(WS, tile_h), bx = make_band(WS, tile_w), uy = make_band(tile_h, WS), ux = make_band(tile_w, WS);
    return ws_layout(n_images, tile_h, tile_w, by.width, bx.width, uy.width, ux.width).total;
}

extern "C" int sq_basic_fit(const void *const *tile_ptrs_dev, const void *tile_base_dev, int64_t tile_stride, int32_t n_images,
                            int32_t tile_h, int32_t tile_w, int32_t tile_pitch, int32_t tile_dtype, float smoothness_flatfield,
                            float *flatfield_dev, void *workspace_dev, int64_t workspace_bytes, sq_basic_info *info,
                            void *stream_) {
    if ((!tile_ptrs_dev && !tile_base_dev) || !flatfield_dev || !workspace_dev)
        return fail(SQ_ERR_INVALID, "sq_basic_fit: NULL argument");
    if (n_images < 1 || n_images > MAX_IMAGES || tile_h < 1 || tile_w < 1 || tile_pitch < tile_w)
        return fail(SQ_ERR_INVALID, "sq_basic_fit: %d images of %dx%d pitch %d (1..%d images)", n_images, tile_h, tile_w, tile_pitch, MAX_IMAGES);
    if (tile_dtype != SQ_U8 && tile_dtype != SQ_U16) return fail(SQ_ERR_UNSUPPORTED, "sq_basic_fit: dtype %d (uint8 / uint16 tiles)", tile_dtype);
    if (!(smoothness_flatfield >= 0.0f)) return fail(SQ_ERR_INVALID, "sq_basic_fit: smoothness_flatfield %g", (double)smoothness_flatfield);
    if (reinterpret_cast<uintptr_t>(workspace_dev) % 256) return fail(SQ_ERR_INVALID, "sq_basic_fit: workspace not 256-byte aligned");
    const int n = n_images;
    const HostBand by = make_band(WS, tile_h), bx = make_band(WS, tile_w), uy = make_band(tile_h, WS), ux = make_band(tile_w, WS);
    const WsLayout L = ws_layout(n, tile_h, tile_w, by.width, bx.width, uy.width, ux.width);
    if (workspace_bytes < L.total) return fail(SQ_ERR_WORKSPACE, "sq_basic_fit: workspace %lld < %lld bytes", (long long)workspace_bytes, (long long)L.total);
    hipStream_t s = static_cast<hipStream_t>(stream_);
    char *ws = static_cast<char *>(workspace_dev);
    auto F = [&](int64_t off) { return reinterpret_cast<float *>(ws + off); };
    auto I = [&](int64_t off) { return reinterpret_cast<int *>(ws + off); };
    Scalars *sc = reinterpret_cast<Scalars *>(ws + L.scalars);
#define SQ_HIP(x)                                                                                  \
    do {                                                                                           \
        hipError_t e_ = (x);                                                                       \
        if (e_ != hipSuccess) return fail(SQ_ERR_HIP, "sq_basic_fit: %s", hipGetErrorString(e_));  \
    } while (0)
    // tables: orthonormal DCT-II matrix (float64 -> float32 like the definition) and the resampling bands
    std::vector<float> cm((size_t)NPIX);
    for (int k = 0; k < WS; ++k)
        for (int j = 0; j < WS; ++j)
            cm[(size_t)k * WS + j] = (float)(k == 0 ? std::sqrt(1.0 / WS) : std::sqrt(2.0 / WS) * std::cos(M_PI * (2 * j + 1) * k / (2.0 * WS)));
    SQ_HIP(hipMemcpyAsync(ws + L.cmat, cm.data(), cm.size() * 4, hipMemcpyHostToDevice, s));
    auto put_band = [&](const HostBand &B, int64_t off_start, int64_t off_w) -> hipError_t {
        hipError_t e = hipMemcpyAsync(ws + off_start, B.start.data(), B.start.size() * 4, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(ws + off_w, B.w.data(), B.w.size() * 4, hipMemcpyHostToDevice, s);
        return e;
    };
    SQ_HIP(put_band(by, L.by_start, L.by_w));
    SQ_HIP(put_band(bx, L.bx_start, L.bx_w));
    SQ_HIP(put_band(uy, L.uy_start, L.uy_w));
    SQ_HIP(put_band(ux, L.ux_start, L.ux_w));
    SQ_HIP(hipStreamSynchronize(s));     // the host vectors above may go now; this entry point synchronises anyway
    const Band dby{I(L.by_start), F(L.by_w), by.width}, dbx{I(L.bx_start), F(L.bx_w), bx.width};
    const Band duy{I(L.uy_start), F(L.uy_w), uy.width}, dux{I(L.ux_start), F(L.ux_w), ux.width};
    if (tile_dtype == SQ_U16)
        hipLaunchKernelGGL(resample_rows_kernel<uint16_t>, dim3(WS, n), dim3(256), 0, s, tile_ptrs_dev, tile_base_dev, tile_stride,
                           tile_pitch, tile_w, dby, F(L.tmp));
    else
        hipLaunchKernelGGL(resample_rows_kernel<uint8_t>, dim3(WS, n), dim3(256), 0, s, tile_ptrs_dev, tile_base_dev, tile_stride,
                           tile_pitch, tile_w, dby, F(L.tmp));
    hipLaunchKernelGGL(resample_cols_kernel, dim3(WS, n), dim3(WS), 0, s, F(L.tmp), tile_w, dbx, F(L.im));
    // norms: spectral norm of the [n x 16384] stack from its Gram matrix, Frobenius norm from the trace
    double *gram_dev = reinterpret_cast<double *>(ws + L.gram);
    hipLaunchKernelGGL(gram_kernel, dim3(n, n), dim3(256), 0, s, F(L.im), n, gram_dev);
    std::vector<double> gram((size_t)n * n);
    SQ_HIP(hipMemcpyAsync(gram.data(), gram_dev, gram.size() * 8, hipMemcpyDeviceToHost, s));
    SQ_HIP(hipStreamSynchronize(s));
    double trace = 0.0;
    for (int i = 0; i < n; ++i) trace += gram[(size_t)i * n + i];
    const double spectral = std::sqrt(largest_eigenvalue(gram, n));
    if (!(spectral > 0.0)) return fail(SQ_ERR_INVALID, "sq_basic_fit: the images are all zero");
    Scalars init{};
    init.image_norm = (double)(float)std::sqrt(trace);
    init.smoothness = smoothness_flatfield;
    SQ_HIP(hipMemcpyAsync(sc, &init, sizeof init, hipMemcpyHostToDevice, s));
    const float init_mu = (float)(MU_COEF / spectral);
    hipLaunchKernelGGL(fill_kernel, dim3(256), dim3(256), 0, s, F(L.wt), (int64_t)n * NPIX, 1.0f);
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(s_dct_shrink_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            DCT_LDS_BYTES) != hipSuccess)
        return fail(SQ_ERR_HIP, "sq_basic_fit: cannot raise the LDS limit");
    int reweights = 0, total_iterations = 0, capped_rounds = 0;
    Scalars host{};
    for (int rw = 0; rw < MAX_REWEIGHT; ++rw) {
        hipLaunchKernelGGL(median_kernel, dim3(NPIX / 256), dim3(256), 0, s, F(L.im), n, F(L.s));
        hipLaunchKernelGGL(solve_init_kernel, dim3(256), dim3(256), 0, s, sc, F(L.b), n, F(L.r), F(L.y), init_mu);
        for (int it = 0; it < MAX_ITER; ++it) {
            hipLaunchKernelGGL(iter_begin_kernel, dim3(1), dim3(1), 0, s, sc, F(L.b), n);
            hipLaunchKernelGGL(s_linear_kernel, dim3(NPIX / 256), dim3(256), 0, s, sc, F(L.im), F(L.r), F(L.y), F(L.b), n, F(L.s), F(L.s_lin));
            hipLaunchKernelGGL(s_dct_shrink_kernel, dim3(1), dim3(1024), DCT_LDS_BYTES, s, sc, F(L.cmat), F(L.s_lin), F(L.s));
            hipLaunchKernelGGL(residual_kernel, dim3(n), dim3(256), 0, s, sc, F(L.im), F(L.r), F(L.y), F(L.wt), F(L.s), F(L.b));
            hipLaunchKernelGGL(multiplier_kernel, dim3(n), dim3(256), 0, s, sc, F(L.im), F(L.r), F(L.y), F(L.s), F(L.b));
            hipLaunchKernelGGL(step_kernel, dim3(1), dim3(1), 0, s, sc);
            if ((it & 15) == 15 || it + 1 == MAX_ITER) {   // converged solves turn the kernels above into no-ops: poll rarely
                SQ_HIP(hipMemcpyAsync(&host, sc, sizeof host, hipMemcpyDeviceToHost, s));
                SQ_HIP(hipStreamSynchronize(s));
                if (host.converged) break;
            }
        }
        total_iterations += host.iterations;
        if (host.iterations >= MAX_ITER) ++capped_rounds;   // the solve stopped at the cap, settled or not
        ++reweights;
        hipLaunchKernelGGL(reweight_s_kernel, dim3(1), dim3(1024), 0, s, sc, F(L.s), F(L.b), n, F(L.last), rw > 0 ? 1 : 0);
        hipLaunchKernelGGL(reweight_w_kernel, dim3(n), dim3(256), 0, s, sc, F(L.r), F(L.s), F(L.b), F(L.wt));
        hipLaunchKernelGGL(reweight_norm_kernel, dim3(256), dim3(256), 0, s, sc, F(L.wt), n);
        SQ_HIP(hipMemcpyAsync(&host, sc, sizeof host, hipMemcpyDeviceToHost, s));
        SQ_HIP(hipStreamSynchronize(s));
        if (rw > 0 && host.mad_den > 0.0 && host.mad_num / host.mad_den <= REWEIGHT_TOL) break;
        SQ_HIP(hipMemcpyAsync(F(L.last), F(L.s), NPIX * 4, hipMemcpyDeviceToDevice, s));
    }
    // A solve that ran into the iteration cap hands back whatever S holds (step_kernel), and a smoothness weight that
    // shrinks every DCT coefficient away leaves S = 0 and 0 / 0 behind it: the gains go to the fusion divide, so a fit
    // whose S is not finite and positive is an error, not a result.  The up-sampling weights are non-negative and every
    // row of them sums to 1, so S > 0 at the working size carries over to every full-size gain.
    std::vector<float> s_host((size_t)NPIX);
    SQ_HIP(hipMemcpyAsync(s_host.data(), F(L.s), s_host.size() * 4, hipMemcpyDeviceToHost, s));
    SQ_HIP(hipGetLastError());
    SQ_HIP(hipStreamSynchronize(s));
    if (info) {
        info->reweight_iterations = reweights;
        info->ladmap_iterations = total_iterations;
        info->working_size = WS;
        info->capped_rounds = capped_rounds;
    }
    int not_finite = 0;
    float s_min = INFINITY;
    for (const float v : s_host) {
        if (!std::isfinite(v)) ++not_finite;
        else s_min = std::min(s_min, v);
    }
    if (not_finite || !(s_min > 0.0f)) {
        char least[64] = "none is finite";
        if (not_finite < NPIX) snprintf(least, sizeof least, "the smallest finite one is %g", (double)s_min);
        return fail(SQ_ERR_NUMERIC,
                    "sq_basic_fit: the fit gave no usable flatfield: %d of %d gains at the working size are not finite, %s (all "
                    "must be > 0); %d of %d re-weighting rounds stopped at the cap of %d iterations%s",
                    not_finite, NPIX, least, capped_rounds, reweights, MAX_ITER,
                    capped_rounds ? " without settling (images too dim or too few, or a smoothness weight that removes the flatfield)" : "");
    }
    hipLaunchKernelGGL(resample_up_kernel, dim3(tile_h), dim3(256), 0, s, F(L.s), tile_h, tile_w, duy, dux, flatfield_dev);
    SQ_HIP(hipGetLastError());
    SQ_HIP(hipStreamSynchronize(s));
#undef SQ_HIP
    return SQ_OK;
}

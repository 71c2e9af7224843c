// The statements of k_prox_wavelet2d / k_prox_wavelet2d_pp (prox_wavelet2d.hip), included INSIDE the kernel bodies that share them (a function shared by two kernels, even a
// forced-inline one, changed the code hipcc generates for the existing kernel; the same tokens do not).
    __shared__ double red[16];
    __shared__ T sig_sh;
    __shared__ T band_sh[kW2dWaves][kW2dBands];
    __shared__ T thr_sh[kW2dBands];
    const int prob = blockIdx.x;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const T* img_in = zin + (size_t)prob * H * W;

    // ---------------- sigma_est = mean over columns of the per-column MAD estimate: prox_tv_regs' sum, wave for wave
    T sigma_est;
    if (sigma_in != nullptr) {
        sigma_est = sigma_in[prob];
    } else {
        constexpr int RPC = H / 4;
        const int cl = lane & 15, q = lane >> 4, ngroups = W / 16;
#pragma unroll 1
        for (int g = wv; g < ngroups; g += kW2dWaves) {
            const T* col = img_in + (size_t)(q * RPC) * W + g * 16 + cl;
            T x[RPC];
#pragma unroll
            for (int i = 0; i < RPC; ++i) x[i] = col[(size_t)i * W];
            const T sc = column_sigma<T, RPC>(x, q);
            double part = q == 0 ? (double)sc : 0.0;
            part = wave_sum(part);
            if (lane == 0) red[g] = part;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0;
            for (int i = 0; i < ngroups; ++i) s += red[i];
            sig_sh = (T)(s / (double)W);
        }
        __syncthreads();
        sigma_est = sig_sh;
    }
    if (sigma_out != nullptr && threadIdx.x == 0) sigma_out[prob] = sigma_est;
    const T sigma = sigma_est > (T)0 ? sigma_est * sigma_modifier : fallback_sigma;
    const T var = sigma * sigma;

    const int lx = lane & 7, ly = lane >> 3;
    const int rcols = (W + 31) / 32, nregions = ((H + 31) / 32) * rcols;

    // ---------------- pass 1: sums of squares of every detail sub-band
    T acc[kW2dBands];
#pragma unroll
    for (int k = 0; k < kW2dBands; ++k) acc[k] = (T)0;
#pragma unroll 1
    for (int r = wv; r < nregions; r += kW2dWaves) {
        const int row0 = (r / rcols) * 32 + ly * 4, col0 = (r % rcols) * 32 + lx * 4;
        const bool inside = row0 < H && col0 < W;      // H, W are multiples of 16: a 4 x 4 block is wholly in or out
        W2dCoef<T> c;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) c.v[i][j] = inside ? img_in[(size_t)(row0 + i) * W + col0 + j] : (T)0;
        w2d_analysis(c, L, lx, ly);
        w2d_accumulate(c, L, lx, ly, inside, acc);
    }
#pragma unroll
    for (int k = 0; k < kW2dBands; ++k) {
        const T s = wave_sum(acc[k]);
        if (lane == 0) band_sh[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 3 * L) {
        const int k = threadIdx.x, l = k / 3 + 1;
        T ss = band_sh[0][k];
        for (int w = 1; w < kW2dWaves; ++w) ss += band_sh[w][k];
        const T dvar = ss / (T)((H >> l) * (W >> l));
        T den = dvar - var;
        den = (den > (T)2.220446049250313e-16 || den != den) ? den : (T)2.220446049250313e-16;   // max(NaN, eps) is NaN
        thr_sh[k] = var / sqrt(den);
    }
    __syncthreads();
    T thr[kW2dBands];
#pragma unroll
    for (int k = 0; k < kW2dBands; ++k) thr[k] = k < 3 * L ? thr_sh[k] : (T)0;

    // ---------------- pass 2: analysis again, shrink, synthesis, store + squared error against the ground truth
    double err = 0.0;
#pragma unroll 1
    for (int r = wv; r < nregions; r += kW2dWaves) {
        const int row0 = (r / rcols) * 32 + ly * 4, col0 = (r % rcols) * 32 + lx * 4;
        const bool inside = row0 < H && col0 < W;
        const size_t off = (size_t)prob * H * W + (size_t)row0 * W + col0;
        W2dCoef<T> c;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) c.v[i][j] = inside ? zin[off + (size_t)i * W + j] : (T)0;
        w2d_analysis(c, L, lx, ly);
        w2d_shrink_synthesis(c, L, lx, ly, thr);
        if (inside) {
            if (xrec != nullptr) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const double df = (double)xrec[off + (size_t)i * W + j] - (double)c.v[i][j];
                        err += df * df;
                    }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) zout[off + (size_t)i * W + j] = c.v[i][j];
        }
    }
    if (sse_out != nullptr) {
        err = wave_sum(err);
        __syncthreads();                               // red[] may still be read by the sigma sum of a slower wave
        if (lane == 0) red[wv] = err;
        __syncthreads();
        if (threadIdx.x == 0) sse_out[prob] = ((red[0] + red[1]) + red[2]) + red[3];
    }

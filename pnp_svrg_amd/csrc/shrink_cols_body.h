// The statements of k_shrink_cols / k_shrink_cols_pp (prox.hip), included INSIDE the kernel bodies that share them (a function shared by two kernels, even a
// forced-inline one, changed the code hipcc generates for the existing kernel; the same tokens do not).
    constexpr int RPC = H / 4;
    const int prob = blockIdx.y, wv = blockIdx.x, lane = threadIdx.x, cl = lane & 15, q = lane >> 4;
    const int nwaves = W / 16;
    T sigma_est;
    if (sigma_in != nullptr) {
        sigma_est = sigma_in[prob];
    } else {
        double s = 0;
        for (int v = 0; v < nwaves; ++v) {                      // k_prox_tv: wave_sum over a wave's 16 columns, waves in order
            double part = lane < 16 ? (double)sig_cols[(size_t)prob * W + v * 16 + lane] : 0.0;
            s += wave_sum(part);
        }
        sigma_est = (T)(s / (double)W);
    }
    if (sigma_out != nullptr && wv == 0 && lane == 0) sigma_out[prob] = sigma_est;
    if (!DENOISE) return;
    const size_t base = (size_t)prob * H * W + (size_t)(q * RPC) * W + wv * 16 + cl;
    T x[RPC];
#pragma unroll
    for (int i = 0; i < RPC; ++i) x[i] = zin[base + (size_t)i * W];
    const T sigma = sigma_est > (T)0 ? sigma_est * sigma_modifier : fallback_sigma;
    haar_bayes_shrink<T, H>(x, sigma * sigma);
    double err = 0.0;
    if (xrec != nullptr) err = (double)column_sq_err<T, RPC>(x, xrec + base, W);
#pragma unroll
    for (int i = 0; i < RPC; ++i) zout[base + (size_t)i * W] = x[i];
    if (sse_out != nullptr) {
        err = wave_sum(err);
        __shared__ bool last;
        if (lane == 0) {
            partial[(size_t)prob * 16 + wv] = err;
            __threadfence();
            last = atomicAdd(&counter[prob], 1u) == (unsigned)(nwaves - 1);
        }
        __syncthreads();
        if (last && lane == 0) {
            __threadfence();
            double s = 0;
            for (int i = 0; i < nwaves; ++i) s += partial[(size_t)prob * 16 + i];
            sse_out[prob] = s;
            counter[prob] = 0;                                  // ready for the next call
        }
    }

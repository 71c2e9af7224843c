// The statements of k_rows_inv / k_rows_inv_pp (csmri_rows.h), included INSIDE the kernel bodies that share them (a function shared by two kernels, even a
// forced-inline one, changed the code hipcc generates for the existing kernel; the same tokens do not).
    using S = FftSmem<T, RA, LA>;
    constexpr int N = S::N, G = S::G, LG = S::LG;
    __shared__ cx<T> smem[S::ELEMS];
    const int t = threadIdx.x, g = t / LG, lane = t % LG;
    const int prob = blockIdx.y, h0 = blockIdx.x * 2 * G;
    if (alpha_vec != nullptr) alpha *= alpha_vec[prob];        // per-problem 1/M0 of a mixed-mask batch

    const int p = t % G;
    cx<T>* zp = smem + p * (N + 1);
    for (int kx = t / G; kx < N / 2; kx += 256 / G) {
        const vec4<T> q = *reinterpret_cast<const vec4<T>*>(S1T + ((size_t)prob * (N / 2) + kx) * H + h0 + 2 * p);
        if (kx == 0) {
            zp[0] = {q.a, q.c};
            zp[N / 2] = {q.b, q.d};
        } else {
            zp[kx] = {q.a - q.d, q.b + q.c};                 // A + iB
            zp[N - kx] = {q.a + q.d, q.c - q.b};             // conj(A) + i conj(B)
        }
    }
    __syncthreads();
    cx<T> v[LG], tw[LG];
    load_twiddles_gen<T, LG>(tw, twtab, lane, N);
#pragma unroll
    for (int r = 0; r < LA; ++r) v[r] = smem[g * (N + 1) + (lane < RA ? lane : 0) + RA * r];
    fft_gen<T, LA, RA, true>(v, tw, smem + g * LG * (LG + 1), lane);

    const size_t ra = (size_t)prob * H * N + (size_t)(h0 + 2 * g) * N, rb = ra + N;
    if (lane < LA) {
#pragma unroll
        for (int r = 0; r < RA; ++r) {
            const int w = lane + LA * r;
            T oa = alpha * v[r].x, ob = alpha * v[r].y;
            if constexpr (MAG) {
                const T pa = c1[ra + w], pb = c1[rb + w];
                oa = sqrt(fma_(oa, oa, pa * pa));
                ob = sqrt(fma_(ob, ob, pb * pb));
            } else {
                if (c1 != nullptr) { oa += beta * c1[ra + w]; ob += beta * c1[rb + w]; }
                if (c2 != nullptr) { oa += gamma * c2[ra + w]; ob += gamma * c2[rb + w]; }
            }
            out[ra + w] = oa;
            out[rb + w] = ob;
        }
    }

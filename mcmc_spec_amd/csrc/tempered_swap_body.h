// tempered_swap_body.h -- the body of tempered_swap_kernel and of its adaptive instantiation (see tempered_step_body.h):
// MSX_TEMPERED_DB(t) is beta[t - 1] - beta[t], formed on the host for a fixed ladder.  TemperedSwapArgs A is the argument.
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = w < A.nw;
    const int ndim = A.ndim;
    for (int t = A.ntemps - 1; t >= 1; --t) {
        bool sw = false;
        if (live) {
#pragma clang fp contract(off)
            const int64_t hi = (int64_t)t * A.nw + w, lo = hi - A.nw;
            const double l_hi = A.ll[hi], l_lo = A.ll[lo];
            const double d = l_hi - l_lo;
            const double lnr = MSX_TEMPERED_DB(t) * d;
            sw = A.logu[(int64_t)(t - 1) * A.nw + w] < lnr;
            if (sw) {
                A.ll[hi] = l_lo;
                A.ll[lo] = l_hi;
                const double p_hi = A.lpr[hi], p_lo = A.lpr[lo];
                A.lpr[hi] = p_lo;
                A.lpr[lo] = p_hi;
                for (int k = 0; k < ndim; ++k) {
                    const double x_hi = A.coords[hi * ndim + k], x_lo = A.coords[lo * ndim + k];
                    A.coords[hi * ndim + k] = x_lo;
                    A.coords[lo * ndim + k] = x_hi;
                }
            }
        }
        const unsigned long long votes = __ballot(sw);
        if ((threadIdx.x & (warpSize - 1)) == 0 && votes != 0ull) atomicAdd(A.nswap + (t - 1), (unsigned long long)__popcll(votes));
    }
    if (!live) return;
    for (int t = 0; t < A.ntemps; ++t) {
        const int64_t i = (int64_t)t * A.nw + w;
        for (int k = 0; k < ndim; ++k) A.chain_row[i * ndim + k] = A.coords[i * ndim + k];
        A.ll_row[i] = A.ll[i];
        A.lpr_row[i] = A.lpr[i];
    }

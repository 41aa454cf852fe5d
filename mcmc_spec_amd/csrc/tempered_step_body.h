// tempered_step_body.h -- the body of tempered_step_kernel and of its adaptive instantiation (tempered_kernels.h includes it
// inside each kernel, with MSX_TEMPERED_BETA(m) defined as the rung's beta): one text, so the fixed run's kernel is compiled
// from exactly the tokens it always was.  TemperedStepArgs A is the kernel's argument.
    const int m = blockIdx.x;
    const int n = A.ns, ndim = A.ndim;
    const int64_t b = (int64_t)m * A.ns, off = (int64_t)m * A.nw;
    const double beta = MSX_TEMPERED_BETA(m);
    if (A.a_on) {
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
#pragma clang fp contract(off)
            const int64_t e = b + i;
            const int64_t si = off + A.a.sidx[e];
            const double pl = A.new_lpr[e], lk = A.new_ll[e];
            const int sp = A.st_lpr[e], sl = A.st_ll[e];
            if (sp > MSX_W_REJECT) atomicMax(A.worst + m, sp);
            if (sp != MSX_W_REJECT && sl > MSX_W_REJECT) atomicMax(A.worst + m, sl);
            const double prod_q = beta * lk;
            const double p_q = pl + prod_q;
            const double old_ll = A.ll[si], old_lpr = A.lpr[si];
            const double prod_s = beta * old_ll;
            const double p_s = old_lpr + prod_s;
            const double lnpdiff = (A.a.fac[e] + p_q) - p_s;
            const bool acc = A.a.logu[e] < lnpdiff;  // NaN differences compare false, like the host loop
            if (acc) {
                for (int d = 0; d < ndim; ++d) A.coords[si * ndim + d] = A.q[e * ndim + d];
                A.ll[si] = lk;
                A.lpr[si] = pl;
                A.nacc[si] = A.nacc[si] + 1;
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    if (A.p_on) {
        const int kind = A.p.kind[m];
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const int64_t e = b + i;
            const int64_t si = off + A.p.sidx[e], c1 = A.p.c1[e], c2 = A.p.c2[e];
            const double g = A.p.g[e];
            for (int d = 0; d < ndim; ++d) {
#pragma clang fp contract(off)
                // no FMA contraction: the bits NumPy's `c - (c - s) * z` and `s + g * (c1 - c2)` give
                const double sv = A.coords[si * ndim + d];
                const double cv = A.coords[c1 * ndim + d];
                double qv;
                if (kind == MSX_MOVE_STRETCH) {
                    const double diff = cv - sv;
                    const double prod = diff * g;
                    qv = cv - prod;
                } else {
                    const double diff = cv - A.coords[c2 * ndim + d];
                    const double prod = g * diff;
                    qv = sv + prod;
                }
                A.q[e * ndim + d] = qv;
            }
        }
    }

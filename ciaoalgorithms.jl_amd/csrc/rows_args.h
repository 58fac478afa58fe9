// rows_args.h -- the argument block of the rows kernels (rows_kernels.h and the families built on it) and the modes it is read in;
// no kernel here, so that launch.h and the API units can name them without seeing one.
#pragma once

#include <stdint.h>

namespace ciao {

enum RowMode {
    RM_GRAD = 0,         // acc += coef(a'x1) * a                                   (+ extra = sum f_i(x1) if want_fval)
    RM_GRAD2 = 1,        // acc += (coef(a'x1) - coef(a'x2)) * a ; extra += hg/gam_i  (LFinito batch, Finito_LFinito.jl:93-98)
    RM_SAGA_INIT = 2,    // table_i = grad f_i(x1) ; acc += table_i                   (SAGA_basic.jl:42-47)
    RM_FINITO_INIT = 3,  // table_i = x1 - (gam_i/N) grad f_i(x1) ; acc += table_i/gam_i   (Finito_basic.jl:77-83)
    RM_FINITO_BATCH = 4, // t = x1 - (gam_i/N) grad f_i(x1) ; acc += (t - table_i)*(hg/gam_i) ; table_i = t  (:110-117)
    RM_AFINITO_INIT = 5  // adaptive Finito init (Finito_adaptive.jl:65-93): table_i = x1; Lipschitz probe at x1 .+ 1 ->
                         // gam_i; meta_i = {c_i, f_i(x1), gam_i, a_i'x1}; acc += x1/gam_i - (c_i/N) a_i; extra += 1/gam_i
};

template <typename T>
struct RowsArgs {
    const T *A;
    const T *b;
    int64_t ld, d;
    int loss;
    T lam;
    int64_t row0, nrows;   // rows row0 .. row0+nrows (idx == nullptr) or idx[0..nrows)
    const int64_t *idx;
    const T *x1, *x2;
    T *table;              // N x d, stride d
    const T *gam;          // per-sample stepsizes (or nullptr -> gam_uniform)
    T gam_uniform;
    T invN;                // 1 / N_total
    T hat_gamma;
    int want_fval;
    T *meta;               // AFINITO_INIT: N x 4 copies x 4 per-sample scalars {c_i, f_i, gam_i, a_i's_i}
    T alpha;               // AFINITO_INIT: the solver's α
    double Nd;             // AFINITO_INIT: N_total as a double (the reference divides a Float64 by the Int N, :88)
    T *rowdot_out;         // GRAD only: if non-null, rowdot_out[row] = a_row'x1 (feeds the SVRG chain, chain_common.h CA_SVRGC)
    T *partial;            // [gridDim.x][pstride]
    int64_t pstride;
    T *pextra;             // [gridDim.x]
    int64_t N;             // local rows (index validation)
    int *errflag;          // device word set to 1 on an out-of-range index
    int small_nb;          // rows_smallm_kernel: tile buffers per wave
};

}  // namespace ciao

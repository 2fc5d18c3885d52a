/*
 * gpx.h -- C-ABI of libgpx: MI355X (gfx950) native GP-regression + uncertainty-propagation core.
 *
 * This is the drop-in boundary for the ONE hot path of snphbaum/scikit-gpuppy
 * (Gram build -> N x N factorisation/solves -> estimate_many -> propagate_GA, fp64,
 * GaussianCovariance).  The reference has no FFI of its own: its "plugin boundary" is the Python
 * operator interface `Covariance` (skgpuppy/Covariance.py:111-359) and the class substitution at
 * import of the propagation classes (skgpuppy/UncertaintyPropagation.py:10-21,244).  A ctypes
 * binding of exactly these entry points is what replaces the numpy/scipy/Cython calls; the
 * reference-side stub a maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.
 *   - all arrays fp64, C-contiguous row-major, caller-owned.  Every `const double*` input and every
 *     output pointer may be a HOST pointer (NumPy buffer) or a DEVICE pointer (HBM-resident buffer,
 *     e.g. a torch tensor's data_ptr): copies use hipMemcpyDefault, device pointers are used in place.
 *   - theta = (log v, log vt, log w_1..w_d) exactly as the reference's theta_min, always a host pointer.
 *   - return 0 = ok; >0 = LAPACK-style info (leading minor not positive definite, also after the
 *     +1e-5*I retry that mirrors skgpuppy/Covariance.py:180-185.  The reference takes that fallback only when its LU
 *     inverse raises; here ANY non-positive pivot of the Cholesky factorisation triggers it -- a numerically indefinite
 *     K that the reference would invert inaccurately gets the documented jitter instead); <0 = bad argument / HIP error
 *     (text via gpx_last_error()).  No exception crosses the ABI.
 *   - a handle is single-owner (one HIP stream, not re-entrant); distinct handles may be used from
 *     distinct threads.  There is NO CPU fallback: without a usable gfx950 device every compute
 *     entry point returns GPX_ERR_NO_DEVICE.
 */
#ifndef GPX_H
#define GPX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPX_ABI_VERSION 1
#define GPX_MAX_D 64          /* largest supported input dimension d */
#define GPX_TILE 128          /* block size of the factorisation (rows are padded to it on device) */

#define GPX_ERR_BAD_ARG   (-1)
#define GPX_ERR_HIP       (-2)
#define GPX_ERR_NO_DEVICE (-3)
#define GPX_ERR_STATE     (-4)
/* value of the device status word of gpx_dev_chol_panel / gpx_dev_chol_panel_next / gpx_dev_chol_panel_split when an in-kernel hand-off of the panel step timed out
 * (GPX_WAIT_LIMIT_MS): the factor is invalid; NOT a non-positive pivot -- never to be answered with the +1e-5 I retry */
#define GPX_INFO_STALLED  0x3fffffff

typedef struct gpx_handle gpx_handle;

/* ---- library ---- */
int         gpx_abi_version(void);
const char *gpx_last_error(void);                 /* thread-local text of the last failure */
int         gpx_device_count(void);               /* number of visible HIP devices (0 if none) */
int         gpx_set_device(int device);           /* device used by handles created afterwards BY THE CALLING THREAD: the choice is
                                                     per host thread (thread-local, default device 0) -- a worker thread that never
                                                     calls it creates its handles on device 0, whatever another thread selected */
int         gpx_pool_trim(void);                  /* release the device buffers cached by the library's allocator */

/* ---- a1/a2: GaussianCovariance.cov_matrix_ij / cov_matrix  (skgpuppy/Covariance.py:461-483) ----
 * K_out[n1,n2] = v exp(-1/2 sum_k w_k (xi_k - xj_k)^2); add_diag (= vt for cov_matrix, 0 for
 * cov_matrix_ij) is added where row == col.  xj may alias xi. */
int gpx_gram(const double *xi, int64_t n1, const double *xj, int64_t n2, int d,
             const double *theta, double add_diag, double *K_out);

/* ---- a4/a5: GaussianProcess.__init__ with theta given + Covariance.inv_cov_matrix
 * (skgpuppy/GaussianProcess.py:19-41, skgpuppy/Covariance.py:167-187) ----
 * Builds K = Gram(x,x) + vt I in HBM, factors it (blocked fp64 Cholesky instead of the reference's
 * LU inverse), solves for alpha = K^-1 t.  t_centered = t - mean(t) (the caller keeps `meant`).
 * On a non-positive pivot the factorisation is repeated once on K + 1e-5 I (reference fallback).
 * stream: a hipStream_t to run on (0 / NULL = the library creates its own). */
int gpx_fit(const double *x, const double *t_centered, int64_t n, int d, const double *theta,
            void *stream, gpx_handle **out);
void gpx_free(gpx_handle *h);

int gpx_n(const gpx_handle *h, int64_t *n, int *d);
int gpx_jitter_used(const gpx_handle *h, double *jitter);   /* 0.0 or 1e-5 */
int gpx_logdet(gpx_handle *h, double *logdet);               /* log det K  (Covariance.py:189-195) */

/* ---- a4 with a caller-supplied matrix: Covariance.inv_cov_matrix(x, theta, cov_matrix=K) (Covariance.py:186-187) ----
 * K [n,n] symmetric positive definite -> Kinv_out [n,n] (Cholesky on the GPU; status > 0 = not PD); logdet_out may be NULL. */
int gpx_spd_inverse(const double *K, int64_t n, double *Kinv_out, double *logdet_out);

/* ---- a4/a5/a6 for ANY Covariance subclass: the operator interface with a SUPPLIED matrix ----
 * The reference's GaussianProcess talks to the operator only through cov.inv_cov_matrix / cov.cov_matrix / cov.cov_matrix_ij
 * (skgpuppy/GaussianProcess.py:39-41, :68-80), and the base-class inv_cov_matrix inverts whatever cov_matrix returns
 * (skgpuppy/Covariance.py:167-187, +1e-5 I retry :180-185).  gpx_fit_matrix is that route on the device: K [n,n] (symmetric, the
 * operator's own cov_matrix(x, theta); host or device pointer) is Cholesky-factored with the same look-ahead schedule and the same
 * single +1e-5 I retry, alpha = K^-1 t_centered is solved.  The handle answers gpx_predict_kv, gpx_alpha, gpx_solve, gpx_chol_mul,
 * gpx_kinv, gpx_chol*, gpx_logdet, gpx_nll, gpx_nll_grad_matrix, gpx_jitter_used; entry points that evaluate the GaussianCovariance
 * kernel itself (gpx_predict, gpx_cjh, gpx_propagate_*, gpx_exact_mean, gpx_nll_grad) return GPX_ERR_STATE on it. */
int gpx_fit_matrix(const double *K, const double *t_centered, int64_t n, void *stream, gpx_handle **out);
/* estimate_many / estimate from the operator's own cross-covariance (GaussianProcess.py:68-80, :94-111): kv [m,n] =
 * cov.cov_matrix_ij(x_star, x), kdiag [m] = diag(cov.cov_matrix(x_star)) (for estimate: cov(x_star, x_star));
 * mean_out[m] = kv alpha (the caller adds `meant`), var_out[m] = kdiag - kv K^-1 kv^T.  Any handle. */
int gpx_predict_kv(gpx_handle *h, const double *kv, int64_t m, const double *kdiag, double *mean_out, double *var_out);

/* ---- a6/a7: GaussianProcess.estimate_many / estimate  (skgpuppy/GaussianProcess.py:68-111) ----
 * mean_out[m] = kv alpha   (the caller adds `meant`),  var_out[m] = v + vt - kv K^-1 kv^T.
 * Never forms the M x M matrices of the reference. */
int gpx_predict(gpx_handle *h, const double *xs, int64_t m, double *mean_out, double *var_out);

/* ---- the predictor's input gradients: d mu / d x* and d sigma^2 / d x* at m queries xs [m, d] ----
 * The reference has no such method: its UncertaintyPropagationLinear differentiates gp(x)[0] by central differences, 2 d calls of
 * estimate per point (skgpuppy/UncertaintyPropagation.py:214-227), and propagates var = sum_k g_k^2 Sigma_kk + vt (:233-242).  Both
 * gradients are closed-form sums: with delta = x_i - x*, c_i the noise-free kernel and d c_i / d x*_k = +w_k delta_k g_i (g = c for
 * GaussianCovariance, skgpuppy/Covariance.py:660-689 -- whose get_Jacobian returns the NEGATIVE of it, as its comment at :687 says --, and
 * G of gpx_matern_* for MaternCovariance, either nu),
 *   d mu / d x*_k = sum_i alpha_i d_k c_i          d sigma^2 / d x*_k = -2 (L^-1 C).(L^-1 d_k c).
 * mean and var are the handle's own predictor's at every query: on a gpx_matern_fit handle they carry the +vt of a query that equals a
 * training row elementwise (Covariance.py:440-451, as gpx_matern_predict), on a gpx_fit handle they do not (as gpx_predict, whose rows
 * are GaussianCovariance.cov_matrix_ij's, :466-483).  No derivative carries that term.  One entry point each for gpx_fit handles and gpx_matern_fit handles of both nu; a periodic or a
 * gpx_fit_matrix handle: GPX_ERR_STATE.  Results do not depend on a query's place in the batch.  m == 0 returns 0. */
/* mean (WITHOUT meant) [m] and its gradient [m, d] from alpha alone: no solve.  Either output may be NULL, not both. */
int gpx_predict_mean_grad(gpx_handle *h, const double *xs, int64_t m, double *mean_out, double *dmean_out);
/* gpx_predict's mean and variance plus both gradients [m, d]; d + 1 solved rows per query.  dmean_out may be NULL. */
int gpx_predict_grad(gpx_handle *h, const double *xs, int64_t m, double *mean_out, double *var_out, double *dmean_out, double *dvar_out);

/* ---- a8: accessors ---- */
int gpx_alpha(gpx_handle *h, double *beta_out);     /* beta = K^-1 t  [n]   (GaussianProcess.py:114-119) */
/* Kinv . B for a few vectors without forming K^-1 (every `numpy.dot(Kinv, v)` of the reference: GaussianProcess.py:77,
 * :116, UncertaintyPropagation.py:412-481).  B [nrhs, n]: the right-hand sides as ROWS.  Linv_B_out = L^-1 B and
 * Kinv_B_out = K^-1 B, both [nrhs, n]; either may be NULL.  Two HBM-bound sweeps over the factor per 32 vectors. */
int gpx_solve(gpx_handle *h, const double *B, int nrhs, double *Linv_B_out, double *Kinv_B_out);
/* "next" row f4, GaussianProcess.get_realisation (skgpuppy/GaussianProcess.py:44-57): out[r] = L Z[r] for the rows of
 * Z [nrhs, n] -- with standard-normal z a draw from N(0, K), K = cov_matrix(x) of the fitted handle (the reference
 * samples the same distribution through numpy's SVD-based multivariate_normal; the random streams differ). */
int gpx_chol_mul(gpx_handle *h, const double *Z, int nrhs, double *out);
int gpx_kinv(gpx_handle *h, double *Kinv_out);      /* K^-1 [n,n], materialised lazily on device
                                                       (GaussianProcess.Kinv attribute, :41, :152-164) */
/* rows [r0, r1) of K^-1 alone: [r1 - r0, n]; r0 a multiple of 128, r1 a multiple of 128 or n.  What a rank of the row-sharded
 * propagation (gpx_propagate_approx_rows / gpx_propagate_exact_rows; the reference's loops over all of Kinv,
 * skgpuppy/UncertaintyPropagation.py:412-481, 343-375, split by rows) builds instead of the whole matrix: E^T L^-T L^-1 for the
 * panel's unit rows, 2 (r1 - r0) N^2 flop and three panel-sized buffers.  The whole matrix is used when it already exists. */
int gpx_kinv_rows(gpx_handle *h, int64_t r0, int64_t r1, double *Kinv_rows_out);
int gpx_chol(gpx_handle *h, double *L_out);         /* lower Cholesky factor [n,n] (zeros above the diagonal) */
int gpx_chol_rows(gpx_handle *h, int64_t r0, int64_t r1, double *L_out);   /* rows [r0,r1) of it: [r1-r0, n] */

/* ---- a9-a11: C_ux / J_ux / H_ux for a propagation input u
 * (skgpuppy/UncertaintyPropagation.py:504-510; Covariance.py:440-451, :660-689) ----
 * C[n] (with the +vt-on-exact-equality quirk), J[n,d] (= J_ux[:, :, 0]), H[n,d,d].  Any of the three
 * may be NULL. */
int gpx_cjh(gpx_handle *h, const double *u, double *C, double *J, double *H);

/* ---- a12: UncertaintyPropagationApprox.propagate_GA / propagate_mean / _getFactor parts
 * (skgpuppy/UncertaintyPropagation.py:386-560, UncertaintyPropagation2.pyx:189-336) ----
 * mean (WITHOUT meant), sigma2 and rest as in _get_sigma2_and_variance_rest; var = sigma2 + rest.
 * Sigma is the full d x d matrix (diagonal used for the J term, full for tr(H Sigma)). */
int gpx_propagate_approx(gpx_handle *h, const double *u, const double *Sigma,
                         double *mean, double *var, double *sigma2, double *rest);

/* The same for b inputs in ONE call (there is no reference counterpart: it replaces a caller's loop over propagate_GA,
 * skgpuppy/UncertaintyPropagation.py:490-523, each turn of which runs :397-481).  U [b, d]; Sigma [b, d, d], or ONE [d, d] matrix
 * for every input when sigma_shared != 0.  Input i's vectors C, tr = tracedot(H, Sigma_i), J_1..J_d are d + 2 right-hand sides of the
 * many-right-hand-side triangular solver of gpx_predict (z_v = L^-1 v; beta.v = z_v.y, v.Kinv v = |z_v|^2, tr.Kinv C = z_tr.z_C):
 * K^-1 is never built and the cache of the single-input calls is left alone.  mean [b] (WITHOUT meant) and var [b] are required,
 * sigma2 [b] and rest [b] may be NULL; host or device pointers.  An input's result does not depend on its place in the batch.
 * b = 0 is a no-op. */
int gpx_propagate_approx_many(gpx_handle *h, const double *U, const double *Sigma, int sigma_shared, int64_t b,
                              double *mean, double *var, double *sigma2, double *rest);

/* Row-sharded form for the multi-GPU host (last row): the 4 + 2 d sums behind gpx_propagate_approx restricted to
 * rows [row0, row1) of K^-1 (row0 a multiple of GPX_TILE, row1 a multiple of GPX_TILE or n).  partial_out [4 + 2 d]:
 * beta.C, beta.tr, C.KinvC, KinvC.tr, then per k: J_k.KinvJ_k, beta.J_k.  The ranks add their partials (ONE all-reduce of
 * 4 + 2 d doubles) and finish on the host: skgpuppy_amd.distributed.combine_approx_partials. */
int gpx_propagate_approx_rows(gpx_handle *h, const double *u, const double *Sigma, int64_t row0, int64_t row1,
                              double *partial_out);

/* Right-hand-side-sharded form (multi-GPU host, no K^-1 on any rank): the share of the same 4 + 2 d sums that the vectors
 * k0 <= k < k1 of [C, J_1..J_d] carry (0: beta.C, beta.tr, C.KinvC, KinvC.tr; k >= 1: J_k.KinvJ_k, beta.J_k), K^-1 v through the
 * two-sweep triangular solver on the rank's copy of the factor; all other entries zero.  One all-reduce, then
 * skgpuppy_amd.distributed.combine_approx_partials as above. */
int gpx_propagate_approx_rhs(gpx_handle *h, const double *u, const double *Sigma, int k0, int k1, double *partial_out);

/* ---- a13: UncertaintyPropagationApprox._get_variance_dv_h for every h in [0,d)
 * (skgpuppy/UncertaintyPropagation.py:564-630, UncertaintyPropagation2.pyx:340-380) ---- */
int gpx_propagate_dvh(gpx_handle *h, const double *u, double *dvh_out /* [d] */);

/* d values of _get_variance_dv_h and _get_sigma2 for b inputs in ONE call (no reference counterpart: it replaces a caller's loop over
 * InverseUncertaintyPropagationApprox.get_best_solution, skgpuppy/InverseUncertaintyPropagation.py:139-173, each turn of which runs
 * skgpuppy/UncertaintyPropagation.py:564-630 d times and :412-481 once).  U [b, d].  Input i's vectors C, J_1..J_d, H_11..H_dd are
 * 2 d + 1 right-hand sides of the many-right-hand-side triangular solver of gpx_predict (z_v = L^-1 v, y = L^-1 t):
 *   dvh_k = -(|z_Jk|^2 - (z_Jk.y)^2) - z_C.z_Hkk  (:564-630)      sigma2 = (v + vt) - |z_C|^2  (:412-433)
 * and the variance rest of a DIAGONAL Sigma = diag(s) is sum_k s_k dvh_k (:435-481, tr(H Sigma) = sum_k H_kk s_k), so _getFactor
 * (:526-560) needs no second call.  K^-1 is neither built nor read and the cache of the single-input calls is left alone.  dvh_out [b, d]
 * is required, sigma2_out [b] may be NULL; host or device pointers.  An input's result does not depend on its place in the batch.
 * b = 0 is a no-op. */
int gpx_propagate_dvh_many(gpx_handle *h, const double *U, int64_t b, double *dvh_out /* [b, d] */, double *sigma2_out /* [b], may be NULL */);

/* ---- numerical propagation: UncertaintyPropagationNumericalHG / UncertaintyPropagationMC
 * (skgpuppy/UncertaintyPropagation.py:90-162 with Utilities.py:144-185) ----
 * Under x ~ N(u, Sigma) the output is the mixture  p(y) = sum_s wq_s N(y; mu(x_s), sigma^2(x_s))  over the nodes x_s = u + A z_s of a
 * Gauss-Hermite grid (A = sqrt(2) times a square root of Sigma, wq = prod w / pi^(d/2)) or of a sample (A a square root of Sigma, wq = 1 / S).
 * b inputs, S nodes each: the rows U_i + A_i z_s (one fma chain over the columns of A_i in increasing order, starting from U_i) go through
 * estimate_many's solver; mom [5, b] = m | var | Ev | m3 | m4 with
 *   m = sum wq mu (WITHOUT meant)   Ev = sum wq sigma^2   var = Ev + sum wq (mu - m)^2   (the central second moment, taken about m)
 *   m3 = sum wq ((mu - m)^3 + 3 (mu - m) sigma^2)   m4 = sum wq ((mu - m)^4 + 6 (mu - m)^2 sigma^2 + 3 sigma^4)
 * -- the mixture's central moments -- and, with ny > 0, dens [b, ny]:  dens[i][j] = p_i(y_j - shift)  (shift = meant evaluates at the
 * caller's y); dens may be NULL when ny == 0.  There is no clamping: a node with sigma^2 <= 0 makes the densities of its input
 * non-finite, as the reference's expression does, and leaves the moments alone.  U [b, d]; A [b, d, d] row-major, or ONE [d, d] when
 * a_shared != 0; z [S, d]; wq [S]; y [b, ny], or ONE [ny] when y_shared != 0.  Gaussian (gpx_fit) and periodic (gpx_periodic_fit) handles;
 * gpx_fit_matrix handles are refused (GPX_ERR_STATE).  The nodes never cross the host, mu and sigma^2 never leave the device.  Host or device
 * pointers.  Bad arguments are refused before anything is queued; b = 0 is a no-op. */
int gpx_propagate_quadrature_many(gpx_handle *h, const double *U, const double *A, int a_shared, int64_t b,
                                  const double *z, const double *wq, int64_t S,
                                  const double *y, int64_t ny, int y_shared, double shift,
                                  double *mom, double *dens);
/* the reduction alone on caller arrays (host or device pointers): mu, var [b, S] are any model's estimate_many output.  No atomics, a fixed
 * summation order: an input's results do not depend on b or on its place in the batch. */
int gpx_mixture_reduce(const double *mu, const double *var, const double *wq, int64_t S, int64_t b,
                       const double *y, int64_t ny, int y_shared, double shift, double *mom, double *dens);
/* test / tool access: the node rows alone, out [b S, d] */
int gpx_quadrature_nodes(const double *U, const double *A, int a_shared, int64_t b, const double *z, int64_t S, int d, double *out);

/* ---- a14: UncertaintyPropagationExact.propagate_GA / propagate_mean
 * (skgpuppy/UncertaintyPropagation.py:246-379, UncertaintyPropagation2.pyx:57-184) ----
 * mean WITHOUT meant; var = (v+vt) - sum_ij (Kinv_ij - beta_i beta_j) L_ij - mean^2. */
int gpx_propagate_exact(gpx_handle *h, const double *u, const double *Sigma, double *mean, double *var);
/* The same for b inputs in ONE call (no reference counterpart: it replaces a caller's loop over propagate_GA).  U [b, d]; Sigma [b, d, d], or
 * ONE [d, d] matrix for every input when sigma_shared != 0; mean [b] (WITHOUT meant) is required, var [b] may be NULL: the means alone, K^-1
 * is then neither built nor read and no GEMM is launched.  Host or device pointers; b = 0 is a no-op.  For inputs that share Sigma the pair
 * weight factorises (a_i = u - x_i, A = Sigma + W^-1 / 2, Ls = sym(2 W - A^-1), F_i = v or v + vt on exact equality):
 *   L_ij / nc2 = h_i(u) h_j(u) E_ij,   h_i(u) = F_i exp(-1/4 a_i^T A^-1 a_i),   E_ij = exp(-1/8 (x_i - x_j)^T Ls (x_i - x_j)),
 *   so the double sum is h^T M h with M = (Kinv - beta beta^T) o E built once per Sigma: one pass over the lower half of K^-1, then
 *   Y = H Lo^T for a slab of inputs on the fp64 GEMM with a triangular B (GPX_GEMM_TRI_B_LOWER) and 2 sum_j Y_ij H_ij per input.
 * With per-input Sigma the batch is cut into runs of consecutive bit-equal Sigma: a run of GPX_EXACT_MANY_MIN_RUN (default 5) inputs or more
 * takes that path, a shorter one the arithmetic of gpx_propagate_exact (the same bits), queued without a synchronisation in between.
 * GPX_EXACT_MANY_SLAB (default 4096, a multiple of 128): inputs per product.  Both are read at every call.  Every Sigma is checked before the
 * first launch (a singular W/2 + Sigma: GPX_ERR_BAD_ARG, nothing written).  An input's result does not depend on its place in the batch; the
 * state of the single-input calls is left alone; the call may build K^-1 on the handle, as gpx_propagate_exact does. */
int gpx_propagate_exact_many(gpx_handle *h, const double *U, const double *Sigma, int sigma_shared, int64_t b, double *mean, double *var);
/* The batched Exact moments WITH their closed-form gradients in u and in the diagonal of Sigma (no reference counterpart: the reference's
 * exact inverse solver runs COBYLA because "Gradient based methods are not suitable ... we would have to calculate the gradient of the GA
 * propagation of the variance", skgpuppy/InverseUncertaintyPropagation.py:103-104; this is that gradient).  U, Sigma, sigma_shared, b as in
 * gpx_propagate_exact_many; mean [b] (WITHOUT meant) and var [b]; dmean_du, dvar_du [b, d]: the derivatives in u_k; dmean_ds, dvar_ds [b, d]:
 * the derivatives in Sigma_kk with every other entry of Sigma held fixed (Sigma itself may be full).  The function differentiated is the one
 * gpx_propagate_exact_many computes: its normalisers read the diagonal of Sigma only, as the reference's do.  Any output may be NULL, but not
 * all four gradients; with var, dvar_du and dvar_ds all NULL, K^-1 is neither built nor read and no GEMM is launched.  With a_j = u - x_j,
 * b_j = A^-1 a_j and the rows h, p_k = h o b_.k, c_k = h o b_.k^2 (2 d + 1 consecutive rows of the product per input), Y_r = Lo r:
 *   S = 2 h.Y_h,  G_k = p_k.Y_h + h.Y_pk,  Q_k = (c_k.Y_h + h.Y_ck) / 2 + p_k.Y_pk,
 *   dvar/du_k = nc2 G_k - 2 m dm/du_k,  dvar/ds_k = -nc2 (Q_k / 2 - w_k / (2 w_k s_k + 1) S) - 2 m dm/ds_k.
 * Per-input Sigma is cut into runs of bit-equal Sigma; EVERY run takes the matrix path, a run of one included.  GPX_EXACT_MANY_SLAB counts
 * product ROWS here: whole inputs go into each slab, and a setting below 2 d + 1 rows is raised to hold one input.  One synchronisation per
 * call; an input's results do not depend on its place in the batch; a singular W/2 + Sigma: GPX_ERR_BAD_ARG, nothing written. */
int gpx_propagate_exact_grad_many(gpx_handle *h, const double *U, const double *Sigma, int sigma_shared, int64_t b, double *mean, double *var,
                                  double *dmean_du, double *dvar_du, double *dmean_ds, double *dvar_ds);
/* row-sharded form (multi-GPU host): partial_out[3] = { sum_{i in rows} beta_i l_i, the rows' share of the double sum / nc2,
 * nc2 }; summed over the row panels: mean = p0, var = v + vt - nc2 p1 - p0^2.  Same row alignment as gpx_propagate_approx_rows. */
int gpx_propagate_exact_rows(gpx_handle *h, const double *u, const double *Sigma, int64_t row0, int64_t row1, double *partial_out);
int gpx_exact_mean(gpx_handle *h, const double *u, const double *Sigma, double *mean);
/* a14 for ANY operator: the reference's UncertaintyPropagationExact.propagate_GA talks to the GP only through _get_beta, _get_W_inv,
 * _inv_cov_matrix, _covariance and x (skgpuppy/UncertaintyPropagation.py:269-290, :323-379), so it runs -- and returns numbers -- for a
 * Covariance subclass with its own kernel.  C_ux [n] = cov(u, x_i) and cuu = cov(u, u) come from the operator's scalar kernel (host,
 * N calls as in the reference), x [n, d] and w [d] = diag(_get_W_inv()) are handle-free HOST arrays, u [d] / Sigma [d, d] host;
 * K^-1 and beta come from h (any fitted handle, e.g. gpx_fit_matrix) or, with h == NULL, from explicit Kinv [n, n] / beta [n].
 * mean WITHOUT meant; var = cuu - sum_ij (Kinv_ij - beta_i beta_j) C_i C_j corr2_ij - mean^2.  var == NULL: the mean alone
 * (propagate_mean(u, Sigma, C_ux), UncertaintyPropagation.py:269-290) -- beta . (C corr), no K^-1 is built or read (Kinv may be NULL). */
int gpx_propagate_exact_matrix(gpx_handle *h, const double *Kinv, const double *beta, const double *x, int64_t n, int d, const double *w,
                               const double *C_ux, const double *u, const double *Sigma, double cuu, double *mean, double *var);
/* the explicit form for MANY calls on one model (an SPGP GP's dense Kinv attribute and beta = Kinv t; any caller-held inverse): Kinv [n, n]
 * and beta [n] are uploaded, padded and symmetrised ONCE (gpx_propagate_exact_matrix with h == NULL does that on every call: N^2 doubles
 * over PCIe each time); then per call only x, C_ux, u, Sigma travel.  Same arithmetic as gpx_propagate_exact_matrix. */
typedef struct gpx_kinv_model gpx_kinv_model;
int  gpx_kinv_model_create(const double *Kinv, const double *beta, int64_t n, gpx_kinv_model **out);
void gpx_kinv_model_free(gpx_kinv_model *m);
int  gpx_propagate_exact_model(gpx_kinv_model *m, const double *x, int d, const double *w, const double *C_ux, const double *u,
                               const double *Sigma, double cuu, double *mean, double *var);

/* ---- Variance decomposition of the predictor mean under independent Gaussian inputs: first-order and total-effect Sobol indices ----
 * No reference counterpart; the closest reference code is the nquad / Hermite-Gauss cross-checks of
 * skgpuppy/UncertaintyPropagation.py:135-210.  x_k ~ N(u_k, s_k) independent, s_k >= 0; mu(x) = sum_i beta_i c_i(x), beta = the handle's
 * alpha, c_i(x) = v exp(-1/2 sum_k w_k (x_k - x_ik)^2) the PLAIN kernel: the +vt of the scalar kernel on elementwise equality is a
 * measure-zero event under a continuous input and does not enter.  Per coordinate k, a_i = u_k - x_ik, om = w_k, sg = s_k:
 *   lm_ik     = -1/2 log1p(om sg) - 1/2 om a_i^2 / (1 + om sg)                                          log E[factor k of c_i]
 *   lE_k(i,j) = -1/2 log1p(2 om sg) - 1/2 om (1 + om sg) / (1 + 2 om sg) (a_i^2 + a_j^2) + om^2 sg / (1 + 2 om sg) a_i a_j
 *             = -1/2 log1p(2 om sg) - 1/4 om (a_i - a_j)^2 - 1/4 om (a_i + a_j)^2 / (1 + 2 om sg)       log E[factor k of c_i c_j] (v-free)
 *   m_k = exp(lm_ik + lm_jk),  E_k = exp(lE_k(i,j)),  b_ij = v^2 beta_i beta_j
 *   mean    = v sum_i beta_i exp(sum_k lm_ik)
 *   V       = sum_ij b_ij (prod_k E_k - prod_k m_k)                    the variance of mu(x)
 *   first_k = sum_ij b_ij (prod_{l != k} m_l) (E_k - m_k)              Var_{x_k}(E[mu | x_k])
 *   total_k = sum_ij b_ij (prod_{l != k} E_l) (E_k - m_k)              E[Var_{x_k}(mu | x_{~k})]
 * Every factor is an expectation of kernel factors in (0, 1]: no exponent is positive (the second way of writing lE_k is the one
 * evaluated).  s_k = 0 gives E_k = m_k: first_k and total_k are then exactly 0.0 (the coordinate is skipped).  sum_k first_k <= V <=
 * sum_k total_k.  It reads (x, beta, v, w) alone -- no K^-1, no factor, no solve -- so it serves gpx_fit handles and pseudo-input handles
 * (gpx_spgp_pseudo_handle) alike, at d exponentials per pair of training points and sweep of 8 coordinates; a Matern, periodic or
 * gpx_fit_matrix handle: GPX_ERR_STATE, the text names the handle's kernel.
 * U [b, d]; S [b, d] variances, or ONE [d] for every input when s_shared != 0; mean [b] (WITHOUT meant), var_mean [b] = V, first [b, d];
 * total [b, d] may be NULL: its sums are then not formed, the other outputs keep their bits.  Host or device pointers.  A negative or
 * non-finite s_k or a null required pointer: GPX_ERR_BAD_ARG before the first launch, nothing written.  b = 0 is a no-op.  Inputs run in
 * chunks sized from the pooled scratch (GPX_SENS_CHUNK, read at every call: at most that many inputs a chunk); no atomics, fixed
 * summation order: an input's result depends neither on its place in the batch nor on the chunking.  A far input (every c_i ~ 1e-130)
 * gives finite, tiny or zero outputs. */
int gpx_sensitivity_many(gpx_handle *h, const double *U, const double *S, int s_shared, int64_t b, double *mean, double *var_mean,
                         double *first, double *total);

/* ---- "next" row f1: hyper-parameter likelihood at the handle's theta
 * (Covariance._negativeloglikelihood / _d_nll_d_theta, skgpuppy/Covariance.py:197-216, :266-282, :605-657) ----
 * nll = N/2 log 2pi + 1/2 log det K + 1/2 t^T K^-1 t ;  grad_out[2+d] = d nll / d theta. */
int gpx_nll(gpx_handle *h, double *nll);
int gpx_nll_grad(gpx_handle *h, double *grad_out);

/* One entry of Covariance._d_nll_d_theta for ANY operator (skgpuppy/Covariance.py:266-282): dK [n,n] = the operator's own
 * _d_cov_matrix_d_theta(x, theta, j); *grad_out = 1/2 tr(K^-1 dK) - 1/2 alpha^T dK alpha in one pass over K^-1 and dK.  Any handle. */
int gpx_nll_grad_matrix(gpx_handle *h, const double *dK, double *grad_out);
/* out[r] = M V[r] for a supplied symmetric matrix M [n,n] and nrhs <= 64 vectors V [nrhs,n] (rows): the device route for the
 * explicit `Kinv` argument of UncertaintyPropagationApprox._get_sigma2 / _get_variance_rest
 * (skgpuppy/UncertaintyPropagation.py:412-481) when it is not the fitted model's own. */
int gpx_symv(const double *M, int64_t n, const double *V, int nrhs, double *out);

/* ---- PeriodicCovariance (skgpuppy/Covariance.py:361-433): ARD squared exponential times a periodic factor per dimension ----
 * theta = (log v, log vt, log w_1..d, log p_1..d, log w2_1..d), 2 + 3 d entries, a host pointer.  With delta = xi - xj
 *   q = 1/2 sum_k [ w_k delta_k^2 + w2_k sin^2(pi delta_k / p_k) ],   k(xi, xj) = v exp(-q) + (vt iff xi == xj in every component).
 * The class inherits the base class's cov_matrix AND cov_matrix_ij (:137-164), so both carry the +vt on exact equality -- also a query
 * row that equals a training row; duplicate training rows make K exactly singular, as in the reference.
 * gpx_periodic_gram replaces those two (deriv = -1) and Covariance._d_cov_matrix_d_theta_ij (:236-253 over :399-433; deriv = j >= 0:
 * d K / d theta_j): out [n1, n2]; xj may alias xi.  K_ij and K_ji are the same bits.  n1, n2 >= 1. */
int gpx_periodic_gram(const double *xi, int64_t n1, const double *xj, int64_t n2, int d, const double *theta, int deriv, double *out);
/* GaussianProcess.__init__ with cov = PeriodicCovariance (skgpuppy/GaussianProcess.py:19-41 over Covariance.py:137-187): K is assembled
 * on the device straight into the factor's buffer (no N x N transfer), then factored with gpx_fit's schedule and its single +1e-5 I
 * retry.  The handle answers whatever a gpx_fit_matrix handle answers (gpx_alpha, gpx_solve, gpx_chol_mul, gpx_kinv*, gpx_chol*,
 * gpx_logdet, gpx_nll, gpx_predict_kv, gpx_nll_grad_matrix, gpx_jitter_used) and the two calls below; the entry points that evaluate the
 * GaussianCovariance kernel (gpx_predict, gpx_cjh, gpx_propagate_*, gpx_exact_mean, gpx_nll_grad) return GPX_ERR_STATE on it, as
 * gpx_periodic_predict / gpx_periodic_nll_grad do on every other handle.  gpx_n reports its d. */
int gpx_periodic_fit(const double *x, const double *t_centered, int64_t n, int d, const double *theta, void *stream, gpx_handle **out);
/* estimate_many / estimate (GaussianProcess.py:68-111): mean_out[m] = kv alpha (WITHOUT meant), var_out[m] = v + vt - kv K^-1 kv^T, kv
 * the cross-covariance with the +vt on equality.  Host or device pointers; m = 0 is a no-op.  A query's result does not depend on its
 * place in the batch or on the chunking (GPX_PERIODIC_CHUNK, read at every call: at most that many queries per chunk, a multiple of 128). */
int gpx_periodic_predict(gpx_handle *h, const double *xs, int64_t m, double *mean_out, double *var_out);
/* Covariance._d_nll_d_theta (Covariance.py:266-282 with PeriodicCovariance._d_cov_d_theta, :399-433): grad_out [2 + 3 d] from ONE pass
 * over the lower half of K^-1 with the kernel recomputed on the fly -- none of the 2 + 3 d derivative matrices is formed.  Fixed-order
 * reduction: two calls give the same bits. */
int gpx_periodic_nll_grad(gpx_handle *h, double *grad_out);

/* ---- MaternCovariance: ARD Matern kernel with nu = 3/2 or 5/2 (nu2 = 2 nu = 3 or 5; anything else: GPX_ERR_BAD_ARG) ----
 * theta = (log v, log vt, log w_1..d), GaussianCovariance's layout, a host pointer.  With delta = xi - xj, q = sum_k w_k delta_k^2 and
 * s = sqrt(2 nu q):   nu = 5/2: Kf = v (1 + s + s^2 / 3) exp(-s),   nu = 3/2: Kf = v (1 + s) exp(-s),
 *   k(xi, xj) = Kf + (vt iff xi == xj in every component, decided on the raw inputs)
 * in cov_matrix AND cov_matrix_ij, as for every kernel built on the base class -- also a query row that equals a training row; the
 * prior variance of a query is v + vt.  delta = 0 gives exactly v (+ vt).
 * gpx_matern_gram: out [n1, n2] = K (deriv = -1) or d K / d theta_deriv (0 <= deriv < 2 + d: Kf | vt on equality | -1/2 w_k delta_k^2 G
 * with G = (5/3) v (1 + s) exp(-s) resp. 3 v exp(-s)); xj may alias xi.  K_ij and K_ji are the same bits.  n1, n2 >= 1. */
int gpx_matern_gram(const double *xi, int64_t n1, const double *xj, int64_t n2, int d, const double *theta, int nu2, int deriv, double *out);
/* GaussianProcess.__init__ with cov = MaternCovariance: K is assembled on the device straight into the factor's buffer, then factored with
 * gpx_fit's schedule and its single +1e-5 I retry.  The handle answers whatever a gpx_fit_matrix handle answers, gpx_propagate_quadrature_many
 * and the gpx_matern_* calls below; the entry points that evaluate the GaussianCovariance kernel and the gpx_periodic_* ones return
 * GPX_ERR_STATE on it, as the gpx_matern_* ones do on every other handle.  gpx_n reports its d. */
int gpx_matern_fit(const double *x, const double *t_centered, int64_t n, int d, const double *theta, int nu2, void *stream, gpx_handle **out);
/* estimate_many / estimate: mean_out[m] = kv alpha (WITHOUT meant), var_out[m] = v + vt - kv K^-1 kv^T, kv the cross-covariance with the
 * +vt on equality, through the routes of gpx_predict.  Host or device pointers; m = 0 is a no-op. */
int gpx_matern_predict(gpx_handle *h, const double *xs, int64_t m, double *mean_out, double *var_out);
/* Covariance._d_nll_d_theta: grad_out [2 + d] from ONE pass over the lower half of K^-1 with the kernel recomputed on the fly.
 * Fixed-order reduction: two calls give the same bits. */
int gpx_matern_nll_grad(gpx_handle *h, double *grad_out);
/* gpx_propagate_approx_many / gpx_propagate_dvh_many (same arguments, same results) for a nu = 5/2 handle, whose kernel is twice
 * differentiable with J_k = -w_k diff_k G and H_kl = (5/3) v exp(-s) [5 (w_k diff_k)(w_l diff_l) - delta_kl w_k (1 + s)], diff = x_i - u.
 * A nu = 3/2 handle (no Hessian at the origin): GPX_ERR_STATE. */
int gpx_matern_propagate_approx_many(gpx_handle *h, const double *U, const double *Sigma, int sigma_shared, int64_t b,
                                     double *mean, double *var, double *sigma2, double *rest);
int gpx_matern_propagate_dvh_many(gpx_handle *h, const double *U, int64_t b, double *dvh_out /* [b, d] */, double *sigma2_out /* [b], may be NULL */);

/* ---- test / tool access: the two kernel stages at the ends of the batched calls (gpx_propagate_approx_many, gpx_propagate_dvh_many,
 * gpx_predict_grad, gpx_matern_propagate_*_many), each alone: no solve in either ---- */
#define GPX_ROWS_APPROX 0   /* d + 2 rows an input: [C, tr, J_1..J_d]          */
#define GPX_ROWS_DVH    1   /* 2 d + 1 rows:        [C, J_1..J_d, H_11..H_dd]  */
#define GPX_ROWS_GRAD   2   /* d + 1 rows:          [C, J_1..J_d]              */
/* or-ed into gpx_rows_reduce's layout: the kernel is launched with its nullable output null (sigma2 of DVH, dmean of GRAD), as
 * gpx_propagate_dvh_many with sigma2_out = NULL and gpx_predict_grad with dmean_out = NULL launch it; that part of out is left as it was */
#define GPX_ROWS_SKIP_NULLABLE 0x100
/* the right-hand-side rows of b inputs as the batched call of this handle's kind would build them (the same launch, from the same
 * dispatch), before any solve: rows_out [round_up(b * nrow, 128), npad], host.  U [b, d]; Sigma [b, d, d], or ONE [d, d] when
 * sigma_shared != 0, read for GPX_ROWS_APPROX alone (may be NULL otherwise).  gpx_fit handles: every layout; gpx_matern_fit with nu = 5/2:
 * every layout, with nu = 3/2: GPX_ROWS_GRAD; every other combination GPX_ERR_STATE.  A batch of more rows than one chunk of the batched
 * calls (32768 rows, fewer from npad = 32768 on), a NULL handle or pointer: GPX_ERR_BAD_ARG before anything is written.  b = 0 is a no-op. */
int gpx_rows_build(gpx_handle *h, int layout, const double *U, const double *Sigma, int sigma_shared, int64_t b, double *rows_out);
/* the row reduction alone on caller arrays (host or device pointers): Zs [b * nrow, npad] (npad a multiple of 128), y [npad]; Sigma as
 * above, read for GPX_ROWS_APPROX alone; out in the layout of the batched calls' device buffer:
 *   APPROX [4, b] = mean | var | sigma2 | rest;   DVH dvh [b, d] then sigma2 [b];   GRAD mean [b] | var [b] | dmean [b, d] | dvar [b, d] */
int gpx_rows_reduce(int layout, int d, int64_t npad, const double *Zs, const double *y, const double *Sigma, int sigma_shared,
                    int64_t b, double vplusvt, double *out);

/* ---- "next" row f3: Snelson sparse pseudo-input GP (SPGPCovariance, skgpuppy/Covariance.py:692-1019) ----
 * theta = [log v, log vt, log w_1..d] (the GaussianCovariance part of the reference's theta), xb = the m x d
 * pseudo-inputs (the tail of the reference's theta, reshaped).  The fit keeps K_NM, chol(K_M + 1e-5 I),
 * Lambda = diag(K_N - Q_N) + vt and chol(B + 1e-5 I), B = K_M + K_MN Lambda^-1 K_NM, on the device: O(N M^2), no N x N
 * matrix.  gpx_spgp_predict returns what GaussianProcess.estimate_many (GaussianProcess.py:68-80) computes with
 * cov = SPGPCovariance: mean = Q_*N Kinv t (WITHOUT meant), var = v + vt - diag(Q_*N Kinv Q_N*), Kinv the Woodbury
 * inverse of :835-863.  gpx_spgp_nll is Snelson's likelihood (:981-1019, jitter 1e-6).  gpx_spgp_dense / _cross
 * materialise cov_matrix(x) (which=0), inv_cov_matrix(x) (which=1) and cov_matrix_ij(xi,xj) for the accessors.
 * Every input (x, xb, the queries) is taken from the first training row before it is scaled: results do not change when all
 * inputs are translated together (exactly so when the translation is exact in fp64). */
typedef struct gpx_spgp gpx_spgp;
int gpx_spgp_fit(const double *x, const double *t_centered, int64_t n, int d, const double *theta, const double *xb,
                 int64_t m, gpx_spgp **out);
void gpx_spgp_free(gpx_spgp *h);
int gpx_spgp_predict(gpx_spgp *h, const double *xs, int64_t ms, double *mean /* [ms] */, double *var /* [ms] */);
int gpx_spgp_nll(gpx_spgp *h, double *nll);
/* analytic d nll / d (log v, log vt, log w_1..d, pseudo-inputs row-major) in O(N m^2): grad_out [2 + d + m d].  Replaces the
 * reference's dense O(N^2 m)-per-parameter gradient (Covariance.py:906-979, not runnable on Python 3).
 * gpx_spgp_nll and gpx_spgp_nll_grad share their common part (the factor of K_M + 1e-6 I, V, gamma, the M x M matrix A and its factor)
 * on the handle: called one right after the other, in either order -- what an optimiser step does (Covariance.py:314-335: ml_estimate hands
 * _negativeloglikelihood and _d_nll_d_theta to L-BFGS-B, which evaluates both at every theta) -- the second call reuses it; any other call in between
 * discards it.  Results do not depend on whether it was reused. */
int gpx_spgp_nll_grad(gpx_spgp *h, double *grad_out);
int gpx_spgp_dense(gpx_spgp *h, int which, double *out /* [n,n] */);
int gpx_spgp_cross(gpx_spgp *h, const double *xi, int64_t n1, const double *xj, int64_t n2, double *out /* [n1,n2] */);
/* *chunks = the number of K-chunks the fit chose for this model's rank-N products (K_MN Lambda^-1 K_NM, A, the gradient's Qb), 0 when each
 * runs as one plain launch.  GPX_SPGP_SPLIT (read at every fit) overrides the choice; a value that does not divide npad / 128 gives 0. */
int gpx_spgp_split(const gpx_spgp *h, int *chunks);
/* The fitted SPGP model as a dense predictor over its m pseudo-inputs: gpx_spgp_predict's mean(x*) = k(x*)^T beta and
 * var(x*) = v + vt - k(x*)^T P k(x*), k(x*) = K(x*, xbar) the plain ARD squared-exponential kernel and
 * P = (K_M + 1e-5 I)^-1 - (B + 1e-5 I)^-1 (m x m), are those of a GP with training inputs xbar, alpha = beta and K^-1 = P.  *out is a
 * gpx_handle of the Gaussian kind with n = m that OWNS copies of xbar, beta and P (built here from the two resident inverse factors:
 * symmetric to the bit, zero in the padding) and has its own stream: it outlives gpx_spgp_free and is released by gpx_free.
 * It has NO factor and no targets.  P is positive semi-definite in exact arithmetic only: it is never factored.  What reads nothing but
 * (xbar, beta, P, v, vt, w) serves it, with the arithmetic and kernels of a gpx_fit handle:
 *   gpx_n, gpx_alpha (beta), gpx_kinv / gpx_kinv_rows (P), gpx_cjh, gpx_exact_mean, gpx_propagate_exact / _exact_rows / _exact_many,
 *   gpx_propagate_approx, gpx_propagate_dvh, gpx_predict_mean_grad, gpx_profile_*;
 *   gpx_propagate_approx_many and gpx_predict_grad in their K^-1 form: the same rows R, Y = R P as one fp64 product per chunk, and the row
 *   reductions on (R, Y, beta): r.y for |L^-1 r|^2, r.beta for (L^-1 r).(L^-1 t).  One synchronisation per chunk, no atomics, results
 *   independent of an input's place in the batch.
 * These are the Gaussian-approximation moments and input gradients of the SPGP predictive distribution itself, at O(m^2) an input; no
 * N x N matrix is formed.  One difference to a gpx_fit handle: a pseudo-input is no observation, so C(u, xbar_i) carries NO +vt where u
 * equals a pseudo-input elementwise (the prior variance stays v + vt).
 * EVERY other entry point that takes a gpx_handle returns GPX_ERR_STATE on it, with a text that names the pseudo-input model: the solves,
 * the factor and likelihood accessors, gpx_predict (use gpx_spgp_predict), gpx_propagate_dvh_many, gpx_propagate_quadrature_many,
 * gpx_propagate_approx_rows / _rhs, gpx_rows_build, gpx_propagate_exact_matrix, gpx_emu_trsm_left. */
int gpx_spgp_pseudo_handle(gpx_spgp *h, gpx_handle **out);

/* ---- measurement: per-kernel-class GPU timings taken with HIP events on the handle's stream ----
 * gpx_profile_enable(h,1) brackets every launch of the listed kernel classes with an event pair;
 * gpx_profile_read sums them (it synchronises the stream).  work = algorithmic flops (GEMM, POTRF,
 * EXACT) or bytes (others) as defined in DESIGN.md. */
enum {
    GPX_K_GRAM = 0,      /* Gram / cross-covariance assembly             (bytes) */
    GPX_K_GEMM = 1,      /* fp64 MFMA GEMM/SYRK/TRSM, 128x128 tiles (dominant) (flops) */
    GPX_K_POTRF_LEAF = 2,/* 128x128 diagonal-block factor + inverse       (flops) */
    GPX_K_TRSV = 3,      /* blocked triangular solves for alpha           (bytes) */
    GPX_K_REDUCE = 4,    /* predictive mean/variance row reductions       (bytes) */
    GPX_K_QUAD = 5,      /* Kinv x V pass of propagate (approx)           (bytes) */
    GPX_K_EXACT = 6,     /* Girard l_i / L_ij double sum                  (flops) */
    GPX_K_GEMM_SMALL = 7,/* the same GEMM kernel in its 64/32-row tile variants (critical-path products) */
    GPX_K_TRSV_RIDE = 8, /* the part of the alpha solve that runs underneath the factorisation's tail (square inverses,
                          * forward substitution of the finished panels): off the critical path, timed under contention */
    GPX_K_GEMM_EMU = 9,  /* estimate_many's deep updates as int8 residue products (split + int8 MFMA + rebuild; fp64-equivalent flops) */
    GPX_K_COUNT = 10
};
/* level 0 = off, 1 = bracket only the dominant kernel (GPX_K_GEMM: 128x128-tile launches), 2 = every class.
 * Environment variable GPX_PROFILE=<level> sets the level of handles at creation (covers gpx_fit itself). */
int gpx_profile_enable(gpx_handle *h, int level);
int gpx_profile_reset(gpx_handle *h);
int gpx_profile_read(gpx_handle *h, int kernel_class, int64_t *launches, double *total_ms, double *total_work);

/* ---- device micro-benchmarks used to re-verify the roofline denominators on the box ---- */
int gpx_bench_mfma_f64(int iters, double *tflops);          /* back-to-back v_mfma_f64_16x16x4_f64 */
/* the int8 residue product of the emulated update alone (rows, cols multiples of 256, K of 128, K < 2^17), random residues,
 * nmod moduli in one launch: mean time per launch */
int gpx_bench_emu_i8(int64_t rows, int64_t cols, int64_t K, int nmod, int iters, double *ms);
/* C[rows, cols] -= A[rows, K] B[cols, K]^T on device buffers (row-major fp64) through the emulated update (Ozaki scheme II on int8
 * matrix cores; GPX_EMU_MODULI moduli).  A, B and C may be windows of larger matrices.  Synchronous.
 * GPX_ERR_BAD_ARG, with text in gpx_last_error() and before anything is allocated, queued or written, unless: K is a multiple of 128
 * below 2^17; lda >= K, ldb >= K, ldc >= cols; lda and ldb are even and A and B 16-byte aligned (the rows are read in pairs of
 * doubles; C needs no more than its natural 8 bytes and ldc may be odd).  rows = 0 or cols = 0 is a valid empty product. */
int gpx_emu_gemm_nt_sub(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t rows, int64_t cols,
                        int64_t K);
/* C[i, j] -= sum_k A[i, k] A[j, k] for j <= i < rows through the emulated update, by column panels of 1024 from ONE residue image of A
 * (every row split once, with the same bit count in either role): the update of the factorisation's deferred columns (DESIGN.md
 * section 5.1).  Nothing above the diagonal is written.  Arguments as gpx_emu_gemm_nt_sub with B = A, cols = rows; tile_rows > 0: a
 * smaller row tile of the image (rounded up to 1024), for tests.  Synchronous. */
int gpx_emu_syrk_lower_sub(const double *A, int64_t lda, int64_t rows, int64_t K, double *C, int64_t ldc, int64_t tile_rows);
/* The same as the factorisation calls it (tests); gpx_emu_syrk_lower_sub is the (diag_tile, plan_rows) = (1, 0) call of it.
 * diag_tile (1, or a power of two that divides 1024): row i ends at the last column of its diag_tile x diag_tile diagonal block, column
 * min(rows - 1, i | (diag_tile - 1)) -- the diagonal blocks are updated in full, above the diagonal too, and nothing else above it is
 * written.  plan_rows (0, or at least rows): when larger than rows, the workspace is planned and allocated for plan_rows rows and planned
 * again for `rows` before the split, the order in which the factorisation reuses one allocation for every later, smaller update; the
 * result does not depend on it.  Other values: GPX_ERR_BAD_ARG before anything is allocated or queued. */
int gpx_emu_syrk_lower_sub_ex(const double *A, int64_t lda, int64_t rows, int64_t K, double *C, int64_t ldc, int64_t tile_rows, int diag_tile,
                              int64_t plan_rows);
/* The two integer kernels of the emulated update alone, on device buffers (tests).  Synchronous.
 * gpx_emu_rebuild: C[rows, cols] -= X 2^-(sa[row] + sb[col]), X the integer in [-P/2, P/2) whose residues modulo the first nmod
 * (2 .. 16) moduli are the bytes R[l * sr + row * ldr + col]; a scale of 0x7fffffff marks a non-finite row or column (NaN).  ldr and sr
 * are multiples of 4 with ldr >= cols rounded up to 4 and sr >= rows * ldr, R is 4-byte aligned, ldc >= cols.
 * gpx_emu_i8_gemm: R_l = (A_l B_l^T) mod p_l as one balanced byte (128 mod 256 stored as -128) for l < nmod (1 .. 16); dense planes
 * A [nmod][rows][K], B [nmod][cols][K], R [nmod][rows][cols]; rows, cols multiples of 256, K of 128 below 2^17, A and B 16-byte aligned. */
int gpx_emu_rebuild(const int8_t *R, int64_t ldr, int64_t sr, int nmod, const int *sa, const int *sb, double *C, int64_t ldc, int64_t rows,
                    int64_t cols);
/* gpx_emu_rebuild with the row end the symmetric update uses: row i is updated up to column min(cols - 1, (i + diag) | dmask) and not
 * beyond (nothing where that is negative); dmask + 1 is a power of two, |diag| <= 2^40.  gpx_emu_rebuild is the (2^40, 0) call of it. */
int gpx_emu_rebuild_ex(const int8_t *R, int64_t ldr, int64_t sr, int nmod, const int *sa, const int *sb, double *C, int64_t ldc, int64_t rows,
                       int64_t cols, int64_t diag, int64_t dmask);
int gpx_emu_i8_gemm(const int8_t *A, const int8_t *B, int64_t rows, int64_t cols, int64_t K, int nmod, int8_t *R);
/* the same with the kernel's strides: planes A [nmod][rows][lda] (lda >= K, a multiple of 16, 255 lda + K < 2^31) and R [nmod][rows][ldr]
 * (ldr >= cols); R and ldr need no alignment (the residues are stored byte by byte).
 * gpx_emu_i8_gemm(A, B, ..., R) is gpx_emu_i8_gemm_ld(A, K, B, ..., R, cols). */
int gpx_emu_i8_gemm_ld(const int8_t *A, int64_t lda, const int8_t *B, int64_t rows, int64_t cols, int64_t K, int nmod, int8_t *R, int64_t ldr);
/* The two splits of the emulated update alone, on device buffers (tests).  Synchronous; GPX_ERR_BAD_ARG before anything is queued.
 * Both store, for every row < rows_pad and l < nmod (1 .. 16), the balanced residue modulo the l-th modulus of a' = rint(x 2^s) as one
 * byte (128 mod 256 stored as -128); rows >= rows are padding (zero residues).  bits is 1 .. 59; X is 16-byte aligned, ldx even.
 * gpx_emu_split: X [rows, K] (ldx >= K; K a multiple of 128 below 2^17) -> res[l * plane + row * K + col], with the row's own scale
 * sig[row] = bits - 1 - ilogb(max |x|) (0 for an all-zero or a padding row); a row that holds a NaN or an Inf gets sig = 0x7fffffff
 * and zero residues.  plane >= rows_pad * K.
 * gpx_emu_split_fixed: X [rows, width] (width a multiple of 16, at most 1024) -> res[l * plane + row * ldr + col] for col < width only
 * (res points at the window's first column; ldr >= width and plane are multiples of 16, res 16-byte aligned), with the given scales
 * sig[row].  An entry with |a'| > 2^bits sets *status to 1 and is stored as 0; a NaN or an Inf sets sig[row] = 0x7fffffff (the row's
 * other entries are still split); a row whose sig is 0x7fffffff at entry is stored as zeros.  *status is never cleared. */
int gpx_emu_split(const double *X, int64_t ldx, int64_t rows, int64_t rows_pad, int64_t K, int bits, int nmod, int8_t *res, int64_t plane,
                  int *sig);
int gpx_emu_split_fixed(const double *X, int64_t ldx, int64_t rows, int64_t rows_pad, int64_t width, int bits, int nmod, int8_t *res,
                        int64_t ldr, int64_t plane, int *sig, int *status);
/* The left-looking form of estimate_many's solve alone (tests): Zs [rows, ldz] <- Z L^-T against the handle's factor (5 slabs of 1024
 * columns or more), device buffers, rows a multiple of 128, ldz >= the padded size and even.  bound [rows] (device): a bound on the
 * magnitude of every entry of the solved row, known before the solve; the residues of a solved slab are split once with the scale it
 * gives.  Z is consumed: afterwards its slab p holds Z_p minus the slab's updates.  tile_rows > 0: a smaller row tile of the residue
 * image.  *status_out != 0: an entry exceeded four times its bound (or a bound was negative or not finite): Zs is not to be used.
 * A row of Z that holds a NaN or an Inf gives NaN from its first affected slab on and raises no status.  Synchronous. */
int gpx_emu_trsm_left(gpx_handle *h, double *Z, int64_t ldz, int64_t rows, const double *bound, double *Zs, int64_t tile_rows, int *status_out);
int gpx_bench_hbm(int64_t bytes, int iters, double *write_gbs, double *copy_gbs);
/* mode 0: MFMA f64 only, 1: VALU v_fma_f64 only, 2: half the waves each; `blocks` workgroups of 4 waves.
 * cycles_per_inst from s_memtime, clock_ghz from s_memtime / s_memrealtime (the clock held under load). */
int gpx_bench_fp64_pipes(int blocks, int iters, int mode, double *tflops, double *cycles_per_inst, double *clock_ghz);

/* ---- building blocks on device pointers (used by the multi-GPU host and by tests) ----
 * All pointers are DEVICE pointers; leading dimensions in elements; sizes multiples of GPX_TILE. */
/* out [rows_pad, cols_pad] in a buffer of leading dimension ld: rows_pad a multiple of 64 and >= n1, cols_pad a multiple of 128 and >= n2;
 * zeros (pad_identity: the identity) outside [n1, n2].  Refused with GPX_ERR_BAD_ARG before anything is queued: a null input with rows,
 * a null output, rows_pad < n1, cols_pad < n2 and padded rows without a single row (n1 == 0 with rows_pad > 0). */
int gpx_dev_gram(const double *xi_dev, int64_t n1, const double *xj_dev, int64_t n2, int d, const double *theta,
                 double add_diag, int lower_only, int pad_identity,
                 double *out_dev, int64_t ld, int64_t rows_pad, int64_t cols_pad, void *stream);
/* the same for inputs already multiplied by sqrt(w) column-wise and resident on the device: one asynchronous launch, no
 * allocation, no synchronisation (v = exp(theta[0])) */
int gpx_dev_gram_scaled(const double *xiw_dev, int64_t n1, const double *xjw_dev, int64_t n2, int d, double v, double add_diag,
                        int lower_only, int pad_identity, double *out_dev, int64_t ld, int64_t rows_pad, int64_t cols_pad,
                        void *stream);
/* C = alpha * A B^T + beta * C  with A[M,K], B[N,K]; lower_only skips tiles above the diagonal */
int gpx_dev_gemm_nt(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc,
                    int64_t M, int64_t N, int64_t K, double alpha, double beta, int lower_only, void *stream);
/* the trailing update of a factorisation panel as ONE launch: C [M, off_cols + M] = alpha A B^T + beta C with A [M, K], B [off_cols + M, K];
 * by 128-tiles, tile row r holds the first off_cols / 128 columns in full and then the lower triangle (r + 1 tiles).  The tiles of the
 * first off_cols columns are computed first and counted per tile column in count_dev[0 .. off_cols / 128) (device ints, zero before the
 * call) as they finish: a consumer on another stream may start on tile column c as soon as count_dev[c] reaches M / 128.  Returns GPX_ERR_STATE (-4) when
 * the shape is too small for this launch. */
int gpx_dev_syrk_trap(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t M, int64_t off_cols,
                      int64_t K, double alpha, double beta, int *count_dev, void *stream);
/* the same with the triangle's columns ending at tri_cols (a multiple of 128 in 0 .. M, else GPX_ERR_BAD_ARG; 0 and M: all of it, the
 * launch above): the near-only update of the factorisation.  Written is C [M, off_cols + tri_cols], by 128-tiles: tile row r holds
 * off_cols / 128 + min(r + 1, tri_cols / 128) tiles -- the first off_cols columns in full, then the lower triangle up to its tile column
 * tri_cols / 128, below which every row holds all tri_cols columns; nothing right of that is read or written.  The counters and
 * GPX_ERR_STATE as above.  gpx_dev_syrk_trap is the tri_cols = 0 call of it. */
int gpx_dev_syrk_trap_cols(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t M, int64_t off_cols,
                           int64_t K, double alpha, double beta, int64_t tri_cols, int *count_dev, void *stream);
/* (lower_only: only the 128-tiles on/below the diagonal of a square C are computed; with N > M the first N - M columns are
 * full and the remaining M x M square is lower-triangular by tiles) */

/* ---- the GEMM's launch forms, one at a time (tests/test_gemm_dispatch.py) ----
 * one triangular operand of a product, square in its own index space: the contraction skips its zero part */
enum {
    GPX_GEMM_TRI_NONE = 0,
    GPX_GEMM_TRI_A_UPPER = 1,   /* A[i][k] = 0 for k < i  (K == M) */
    GPX_GEMM_TRI_A_LOWER = 2,   /* A[i][k] = 0 for k > i  (K == M) */
    GPX_GEMM_TRI_B_LOWER = 3,   /* B[j][k] = 0 for k > j  (K == N) */
    GPX_GEMM_TRI_B_UPPER = 5    /* B[j][k] = 0 for k < j  (K == N); 4 and 6 are internal */
};
/* which launch gpx_dev_gemm_nt_ex chose: block tile rows / 32, block tile columns / 32, lower-only or plain, and for a triangular B
 * the form of its tile enumeration */
#define GPX_GEMM_VARIANT(wm, wn, lower, form) ((wm) | ((wn) << 4) | ((lower) << 8) | ((form) << 12))
enum { GPX_GEMM_FORM_NONE = 0, GPX_GEMM_FORM_FINE = 1, GPX_GEMM_FORM_LONGEST_FIRST = 2, GPX_GEMM_FORM_PAIRED = 3, GPX_GEMM_FORM_SMALL = 4 };
enum {
    GPX_GEMM_V_NONE = 0,                                              /* nothing was launched (refused, or an empty product) */
    GPX_GEMM_V_128X128 = GPX_GEMM_VARIANT(4, 4, 0, 0),                /* the bulk launch: grouped walk, one chunk per XCD */
    GPX_GEMM_V_64X64 = GPX_GEMM_VARIANT(2, 2, 0, 0),                  /* fewer than 192 tiles, or small_tiles */
    GPX_GEMM_V_64X128 = GPX_GEMM_VARIANT(2, 4, 0, 0),                 /* one column tile, 96 row tiles or more */
    GPX_GEMM_V_32X128 = GPX_GEMM_VARIANT(1, 4, 0, 0),                 /* one column tile, fewer */
    GPX_GEMM_V_LOWER_128X128 = GPX_GEMM_VARIANT(4, 4, 1, 0),
    GPX_GEMM_V_LOWER_64X64 = GPX_GEMM_VARIANT(2, 2, 1, 0),
    GPX_GEMM_V_LOWER_32X32 = GPX_GEMM_VARIANT(1, 1, 1, 0),            /* at most 40 tiles with 512 <= K <= 2048 */
    GPX_GEMM_V_TRIB_FINE = GPX_GEMM_VARIANT(2, 2, 0, 1),              /* triangular B, 192 .. 447 tiles: 64 x 64 tiles, longest first */
    GPX_GEMM_V_TRIB_LONGEST_FIRST = GPX_GEMM_VARIANT(4, 4, 0, 2),     /* triangular B: 128 x 128 tiles, longest first */
    GPX_GEMM_V_TRIB_PAIRED = GPX_GEMM_VARIANT(4, 4, 0, 3),            /* triangular B: column tiles bx and ncols - 1 - bx in one workgroup */
    GPX_GEMM_V_TRIB_SMALL_64X64 = GPX_GEMM_VARIANT(2, 2, 0, 4),       /* triangular B, fewer than 192 tiles: the tile the plain rules give */
    GPX_GEMM_V_TRIB_SMALL_64X128 = GPX_GEMM_VARIANT(2, 4, 0, 4),
    GPX_GEMM_V_TRIB_SMALL_32X128 = GPX_GEMM_VARIANT(1, 4, 0, 4)
};
/* gpx_dev_gemm_nt with the launcher's remaining arguments:
 *   ktrim != 0, lower_only (square C, K == M): BOTH operands are upper triangular (operand[i][k] = 0 for k < i), tile row by contracts
 *     over k >= by * (tile rows) only;
 *   ktrim != 0, plain: A alone is upper triangular with its diagonal ktrim - 1 columns to the left of its first column (A[i][k] = 0
 *     for k < i - (ktrim - 1)); ktrim - 1 a multiple of 16;
 *   tri: one of GPX_GEMM_TRI_* (plain launches, no ktrim); the internal values are refused with GPX_ERR_BAD_ARG;
 *   small_tiles: 64 x 64 block tiles also where the product has 192 tiles or more;
 *   variant_out: HOST int, may be NULL; receives the GPX_GEMM_V_* code of the launch that was chosen.
 * Read contract of an operand declared triangular or shortened by ktrim: by 128 x 128 tiles of the operand (tile row = rows / 128, tile
 * column = k / 128), a launch reads NOTHING in the tiles that lie wholly inside the zero part -- they may hold anything, NaN included --
 * and inside the tiles that the diagonal crosses the CALLER supplies the zeros.  (gpx_adopt_factor relies on this: the strictly-upper
 * tiles of L are scratch.) */
int gpx_dev_gemm_nt_ex(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t M, int64_t N, int64_t K,
                       double alpha, double beta, int lower_only, int ktrim, int tri, int small_tiles, int *variant_out, void *stream);
/* C [M, N] = alpha A B^T with B lower triangular (K == N, read contract as above) on 128 x 128 tiles, M / 128 * N / 128 >= 192 of them,
 * and of every row the partial sums over each 64-column piece c: p2[row * nslots + slot0 + c] = sum C[row][64 c + j]^2,
 * py[row * nslots + slot0 + c] = sum C[row][64 c + j] y[64 c + j]; y [N], p2 and py [M, nslots] with nslots >= slot0 + N / 64.  No other
 * slot is written. */
int gpx_dev_gemm_nt_tri_reduce(const double *A, int64_t lda, const double *B, int64_t ldb, double *C, int64_t ldc, int64_t M, int64_t N,
                               double alpha, const double *y, double *p2, double *py, int64_t slot0, int64_t nslots, void *stream);
/* `batch` independent products C_z = alpha A_z B_z^T + beta C_z on 64 x 64 tiles (M, N multiples of 64): problem z = (p, q) with
 * q = z % nq has its operands at A + p a_sp + q a_sq, B + p b_sp + q b_sq, C + p c_sp + q c_sq (elements; the A and B strides even).
 * tri: GPX_GEMM_TRI_* of every problem (then M == N == K). */
int gpx_dev_gemm_nt_batched(const double *A, int64_t lda, int64_t a_sp, int64_t a_sq, const double *B, int64_t ldb, int64_t b_sp,
                            int64_t b_sq, double *C, int64_t ldc, int64_t c_sp, int64_t c_sq, int nq, int tri, int64_t M, int64_t N,
                            int64_t K, double alpha, double beta, int64_t batch, void *stream);
/* split-K SYRK as one launch: parts [nchunks, m, m] (dense), the lower 128 x 128 tiles of parts[c] = alpha W_c W2_c^T with
 * W_c = W[:, c kchunk : (c + 1) kchunk); W [m, nchunks kchunk] with leading dimension ldw, W2 the same shape and leading dimension or
 * NULL (= W).  The tiles above the diagonal of every part are not written. */
int gpx_dev_syrk_splitk(const double *W, int64_t ldw, const double *W2, double *parts, int64_t m, int64_t kchunk, int nchunks,
                        double alpha, void *stream);
/* factor one 128x128 diagonal block in place (lower) and write its inverse to dinv[128*128];
 * info_dev: device int, set to 1-based failing column + col_offset on a non-positive pivot */
int gpx_dev_potrf_leaf(double *A, int64_t ld, double *dinv, double *diag_out, int *info_dev, int col_offset, void *stream);

/* factor block columns [B0,B1) (units of GPX_TILE) of the row-major matrix L (ld, nblk block rows), all updates
 * from columns < B0 already applied: the diagonal square on `stream` (128 columns at a time, or -- first panel, short trailing
 * matrix -- as one square launch of the dataflow kernel), the rows below it solved column by column on an internal side stream
 * alongside that chain (forked from and joined back into `stream`).  This is the per-panel step the multi-GPU host
 * (skgpuppy_amd/distributed.py) runs on the panel owner.  *info_dev: 0, the 1-based failing column, or GPX_INFO_STALLED. */
int gpx_dev_chol_panel(double *L, int64_t ld, int64_t nblk, int64_t B0, int64_t B1, double *dinv, double *diag,
                       int *info_dev, void *stream);
/* the same, preceded by the rank-kp update with the PREVIOUS panel that the block columns [B0,B1) still lack:
 * prev = its rows from B0 * GPX_TILE down ([rows, kp], leading dimension ldp; it may live in L or in a receive buffer).  The
 * diagonal square is updated first so that the chain starts at once; the rows below are updated on the side stream ahead
 * of the column solves (the look-ahead order of the single-GPU factorisation). */
int gpx_dev_chol_panel_next(double *L, int64_t ld, int64_t nblk, int64_t B0, int64_t B1, const double *prev, int64_t ldp,
                            int64_t kp, double *dinv, double *diag, int *info_dev, void *stream);
/* the same step for a panel whose message travels in TWO parts (skgpuppy_amd/distributed.py, split panel message): the rows below
 * the square are cut into a HEAD -- the first head_blocks block rows, i.e. the NEXT panel's diagonal square, all its owner needs to start
 * its own chain -- solved on stream_head, and the rest on stream_far; both trail the chain on `stream` column by column.  prev may be
 * NULL (first panel: no update).  The two row streams are ordered behind `stream` as it stands at the call and are NOT joined back:
 * after the call `stream` carries the square, dinv and diag, stream_head the head rows, stream_far the far rows -- each part can be
 * packed and sent as soon as ITS stream gets there.  Whatever else the row updates need (the arrival of prev's far rows) the caller
 * orders on stream_head / stream_far before the call.  Three distinct streams; head and far must not be the null stream.
 * Same arithmetic per tile as gpx_dev_chol_panel_next (the slices only regroup rows): bit-identical factor.
 * Part of the multi-GPU form of skgpuppy/Covariance.py:179 (the reference factors on one host with scipy/LAPACK). */
int gpx_dev_chol_panel_split(double *L, int64_t ld, int64_t nblk, int64_t B0, int64_t B1, int64_t head_blocks, const double *prev,
                             int64_t ldp, int64_t kp, double *dinv, double *diag, int *info_dev, void *stream, void *stream_head,
                             void *stream_far);
/* how many ranks share the trailing update that the CALLING THREAD's owner steps (gpx_dev_chol_panel / _next / _split) run beside; default 1.
 * The step factors its diagonal square as ONE square launch of the dataflow kernel when the trailing update is short (fewer than 1000
 * tiles) -- at R ranks that is decided on the tiles divided by R, an owner's chain running next to 1 / R of the update.  Set by the
 * multi-GPU hosts (skgpuppy_amd/distributed.py, gpx_multi_fit); same arithmetic either way (bit-identical factor). */
int gpx_dev_set_panel_share(int ranks);
/* the factorisation (first_block = 0) or its trailing part (all updates from the block columns before first_block applied; first_block
 * a multiple of 8) as ONE persistent dataflow launch (csrc/dflow.hip): leaf, column solves, in-panel and trailing updates are tasks that
 * resident workgroups hand to each other through agent-scope counters instead of ~24 dependent launches per 1024-column panel.  This is what
 * gpx_fit runs for the trailing panels of its Cholesky (replaces skgpuppy/Covariance.py:179); exported for tests and probes.  Synchronous.
 * info_dev: two device ints, zero before the call: [0] potrf status (1-based failing column), [1] set when an in-kernel wait expired. */
int gpx_dev_chol_dataflow(double *L, int64_t ld, int64_t nblk, int64_t first_block, double *dinv, double *diag, int *info_dev, void *stream);
/* build a handle around an EXISTING factor in HBM (L [npad,npad] with ld == npad, dinv [npad/128,128,128],
 * diag [npad]; the caller keeps ownership and must keep them alive): solves for alpha; predict / propagate as usual.
 * The strictly-upper 128x128 tiles of L_dev are scratch for the library (the first Approx propagation stores L^T there).
 * Used by the sharded fit, where every rank ends up with the full factor after the panel broadcasts. */
int gpx_adopt_factor(const double *x, const double *t_centered, int64_t n, int d, const double *theta, double *L_dev,
                     double *dinv_dev, double *diag_dev, double jitter, void *stream, gpx_handle **out);


/* ---- e1-e4 behind the C-ABI: ONE host process driving several devices of one node (csrc/multi.hip) ----
 * The reference has no distributed code (it factors on one host: skgpuppy/Covariance.py:179, and predicts with two dense products:
 * skgpuppy/GaussianProcess.py:75-78); SURVEY.md 8b proposed gpx_set_devices(...) / a multi-GPU handle for the sharded path.  This is that
 * handle -- the schedule of skgpuppy_amd/distributed.py (one process per GPU, torch.distributed) for callers without Python or a process
 * launcher: sharded K-build, panel Cholesky with look-ahead and peer-to-peer panel messages, query-sharded estimate_many,
 * right-hand-side-sharded propagate_GA.  devices[ndev]: HIP device ordinals, block-cyclic owners of the 1024-column panels; an ordinal may
 * repeat (several logical ranks on one GPU: how the path is tested on a one-GPU box).  x [n, d], t_centered [n], theta [2 + d]: HOST
 * arrays.  Every device ends with the complete factor (npad^2 doubles each).  Status as gpx_fit: > 0 = not positive definite also after
 * the ONE collective retry on K + 1e-5 I (Covariance.py:180-185); a timed-out in-kernel hand-off is GPX_ERR_STATE, never jitter.
 * Not thread-safe per handle; distinct handles may be used from distinct threads. */
typedef struct gpx_multi gpx_multi;
int  gpx_multi_fit(const double *x, const double *t_centered, int64_t n, int d, const double *theta, const int *devices, int ndev,
                   gpx_multi **out);
void gpx_multi_free(gpx_multi *m);
int  gpx_multi_info(const gpx_multi *m, int *ndev, int64_t *npanels, double *jitter_used);
/* beta = K^-1 t (GaussianProcess.py:114-119), from the first device's copy of the factor */
int  gpx_multi_alpha(gpx_multi *m, double *beta_out);
/* GaussianProcess.estimate_many (GaussianProcess.py:68-80) with the queries dealt to the devices in contiguous shards, no exchange;
 * xs [m, d], mean_out / var_out [m] HOST arrays; mean WITHOUT meant */
int  gpx_multi_predict(gpx_multi *m, const double *xs, int64_t nq, double *mean_out, double *var_out);
/* UncertaintyPropagationApprox.propagate_GA (UncertaintyPropagation.py:397-479): the d + 1 right-hand sides [C, J_1..J_d] dealt to the
 * devices (gpx_propagate_approx_rhs on each), the 4 + 2 d partial sums added on the host; outputs as gpx_propagate_approx (mean WITHOUT
 * meant; sigma2 / rest optional) */
int  gpx_multi_propagate_approx(gpx_multi *m, const double *u, const double *Sigma, double *mean, double *var, double *sigma2, double *rest);
/* UncertaintyPropagationExact.propagate_GA (UncertaintyPropagation.py:246-379): row panels of equal triangle area, one per device
 * (gpx_propagate_exact_rows: each device builds only its rows of K^-1), two partial sums added on the host; mean WITHOUT meant */
int  gpx_multi_propagate_exact(gpx_multi *m, const double *u, const double *Sigma, double *mean, double *var);

#ifdef __cplusplus
}
#endif
#endif /* GPX_H */

// Part of capi.hip (included there: one translation unit, so the file-local helpers of capi.hip, capi_fused.inl and capi_phase.inl are
// in scope) -- power spectrum, cross-spectrum and coherence (spectrum.hip): the trial-averaged power of a resident or host field under
// a spectral operator, and the cross-spectral matrix and coherence of all site pairs from its stored coefficients.

// (checked before anything is read; as analytic_check with M = R * S, plus the outputs' own counts)
static void power_check(const char *who, int nz, int nts, int R, int S, int nrow) {
    GP_REQUIRE(nz > 0 && nts > 0 && R > 0 && S > 0 && nrow > 0, -3, "%s: bad arguments", who);
    const long M = (long)R * S;
    GP_REQUIRE(M < GPCSD_MAX_GEMM_LD_KMAJOR && nts < (1 << 22) && (long)nz * M < (1L << 31) && (long)nz * M * nrow / 64 < (1L << 31) &&
                   (long)nrow * nts < (1L << 28) && (double)nz * nrow * S * power_slots(M) < 1099511627776.0,
               GPCSD_ERR_CAPACITY, "%s: R * S = %ld (or nts = %d, or nz * R * S = %ld, or nrow * nts >= 2^28, or the partial sums) exceeds the "
               "capacity of one operand row (%ld doubles; GPCSD_MAX_GEMM_LD_KMAJOR)", who, M, nts, (long)nz * M, (long)GPCSD_MAX_GEMM_LD_KMAJOR);
}

extern "C" int gpcsd_power_spectrum(gpcsd_ctx *c, const double *x, int nz, int nts, int R, int S, const double *A_re, const double *A_im,
                                    int nrow, double *psd, double *power, double *X_re, double *X_im) {
    GP_API_BEGIN(c)
    GP_REQUIRE(x && A_re && A_im && psd, -3, "power_spectrum: bad arguments");
    power_check("power_spectrum", nz, nts, R, S, nrow);
    const size_t M = (size_t)R * S, nin = (size_t)nz * nts * M, nout = (size_t)nz * nrow * M, npsd = (size_t)nz * nrow * S;
    PowerDesc d;
    d.X = c->upload<double>("op_in0", x, nin);
    d.Are = c->upload<double>("op_in1", A_re, (size_t)nrow * nts);
    d.Aim = c->upload<double>("op_in2", A_im, (size_t)nrow * nts);
    d.nz = nz; d.nts = nts; d.R = R; d.S = S; d.nrow = nrow;
    double *const host[3] = {power, X_re, X_im};
    double **const dev[3] = {&d.power, &d.re, &d.im};
    int nwant = 0;
    for (int k = 0; k < 3; ++k) nwant += host[k] != nullptr;
    double *dO = c->buf<double>("op_out", npsd + nout * (size_t)nwant);
    d.psd = dO;
    for (int k = 0, at = 0; k < 3; ++k)
        if (host[k]) *dev[k] = dO + npsd + nout * (size_t)at++;
    d.part = c->buf<double>("spec_part", npsd * (size_t)power_slots((long)M));
    k_power(c, d, c->stream);
    c->download(psd, d.psd, npsd * sizeof(double));
    for (int k = 0; k < 3; ++k)
        if (host[k]) c->download(host[k], *dev[k], nout * sizeof(double));
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_power_spectrum_resident(gpcsd_ctx *c, const char *src_name, long src_offset, int nz, int nts, int R, int S,
                                             const double *A_re, const double *A_im, int nrow, int want_mask) {
    GP_API_BEGIN(c)
    static const char *const out_name[3] = {"spec_power", "spec_re", "spec_im"};
    GP_REQUIRE(src_name && A_re && A_im && src_offset >= 0 && want_mask >= 0 && want_mask < 8, -3, "power_spectrum_resident: bad arguments");
    power_check("power_spectrum_resident", nz, nts, R, S, nrow);
    for (const char *n : {"spec_psd", "spec_power", "spec_re", "spec_im", "spec_part"})
        GP_REQUIRE(strcmp(src_name, n) != 0, -3, "power_spectrum_resident: '%s' is one of the call's outputs", n);
    auto it = c->bufs.find(src_name);
    GP_REQUIRE(it != c->bufs.end() && it->second.p, -2, "power_spectrum_resident: no device buffer named '%s'", src_name);
    const size_t M = (size_t)R * S, nin = (size_t)nz * nts * M, nout = (size_t)nz * nrow * M, npsd = (size_t)nz * nrow * S;
    GP_REQUIRE(((size_t)src_offset + nin) * sizeof(double) <= it->second.bytes, -3,
               "power_spectrum_resident: '%s' holds %zu bytes, offset %ld + %zu doubles asked for", src_name, it->second.bytes, src_offset, nin);
    // a queued prediction that still owes its status produced the source: collected first, as gpcsd_fetch does
    if (int rc = drain_async(c)) return rc;
    PowerDesc d;
    d.X = static_cast<const double *>(it->second.p) + src_offset;
    d.Are = c->upload<double>("spec_A_re", A_re, (size_t)nrow * nts);
    d.Aim = c->upload<double>("spec_A_im", A_im, (size_t)nrow * nts);
    d.nz = nz; d.nts = nts; d.R = R; d.S = S; d.nrow = nrow;
    d.psd = c->buf<double>("spec_psd", npsd);
    d.part = c->buf<double>("spec_part", npsd * (size_t)power_slots((long)M));
    double **const dev[3] = {&d.power, &d.re, &d.im};
    for (int k = 0; k < 3; ++k)
        if (want_mask & (1 << k)) *dev[k] = c->buf<double>(out_name[k], nout);
    c->spec_shape[0] = c->spec_shape[1] = c->spec_shape[2] = c->spec_shape[3] = 0;      // (until both halves of the coefficients are in place)
    k_power(c, d, c->stream);
    c->sync();
    if ((want_mask & 6) == 6) {
        c->spec_shape[0] = nz; c->spec_shape[1] = nrow; c->spec_shape[2] = R; c->spec_shape[3] = S;
    }
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

// Sx = 1/R sum_r X_a conj(X_b) is plv_kernel on the coefficients in place of unit phasors; the coherence follows from its two parts
static void cross_spectrum_run(gpcsd_ctx *c, const double *xre, const double *xim, int nz, int nrow, int R, int S, double *sre, double *sim,
                               double *coh) {
    PlvDesc d;
    d.ure = xre; d.uim = xim;
    d.nz = nz; d.nsel = nrow; d.R = R; d.S = S;
    d.cre = sre; d.cim = sim;
    k_plv(c, d, c->stream);
    if (coh) k_coherence(c, sre, sim, coh, nz, (long)S * nrow, c->stream);
}

extern "C" int gpcsd_cross_spectrum(gpcsd_ctx *c, const double *X_re, const double *X_im, int nz, int nrow, int R, int S, double *s_re,
                                    double *s_im, double *coh) {
    GP_API_BEGIN(c)
    GP_REQUIRE(X_re && X_im, -3, "cross_spectrum: bad arguments");
    plv_check("cross_spectrum", nz, nrow, R, S);
    const size_t nin = (size_t)nz * nrow * R * S, nout = (size_t)S * nrow * nz * nz;
    const double *dre = c->upload<double>("op_in0", X_re, nin);
    const double *dim = c->upload<double>("op_in1", X_im, nin);
    double *dO = c->buf<double>("op_out", nout * 3);
    cross_spectrum_run(c, dre, dim, nz, nrow, R, S, dO, dO + nout, coh ? dO + 2 * nout : nullptr);
    double *const host[3] = {s_re, s_im, coh};
    for (int k = 0; k < 3; ++k)
        if (host[k]) c->download(host[k], dO + nout * (size_t)k, nout * sizeof(double));
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_cross_spectrum_resident(gpcsd_ctx *c, int nz, int nrow, int R, int S) {
    GP_API_BEGIN(c)
    plv_check("cross_spectrum_resident", nz, nrow, R, S);
    GP_REQUIRE(c->spec_shape[0] == nz && c->spec_shape[1] == nrow && c->spec_shape[2] == R && c->spec_shape[3] == S, -4,
               "cross_spectrum_resident: no gpcsd_power_spectrum_resident call has left coefficients of shape (%d, %d, %d, %d) (found "
               "(%ld, %ld, %ld, %ld))", nz, nrow, R, S, c->spec_shape[0], c->spec_shape[1], c->spec_shape[2], c->spec_shape[3]);
    const size_t nout = (size_t)S * nrow * nz * nz;
    const double *xre = static_cast<const double *>(c->bufs["spec_re"].p), *xim = static_cast<const double *>(c->bufs["spec_im"].p);
    double *sre = c->buf<double>("xspec_re", nout), *sim = c->buf<double>("xspec_im", nout), *coh = c->buf<double>("xspec_coh", nout);
    cross_spectrum_run(c, xre, xim, nz, nrow, R, S, sre, sim, coh);
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

// Part of capi.hip (included there: one translation unit, so the file-local helpers of capi.hip and capi_fused.inl are in scope) --
// band phase and phase-locking value (phase.hip): the analytic signal of a resident or host field under a complex operator, and the
// PLV of all site pairs from its unit phasors.

// (checked before anything is read: M is the row length of the field's planes, the K-major operand of the product; the counts
// index the grid and the outputs)
static void analytic_check(const char *who, int nz, int nts, long M, int nsel) {
    GP_REQUIRE(nz > 0 && nts > 0 && M > 0 && nsel > 0, -3, "%s: bad arguments", who);
    GP_REQUIRE(M < GPCSD_MAX_GEMM_LD_KMAJOR && nts < (1 << 22) && (long)nz * M < (1L << 31) && (long)nz * M * nsel / 64 < (1L << 31) &&
                   (long)nsel * nts < (1L << 28),
               GPCSD_ERR_CAPACITY, "%s: M = %ld (or nts = %d, or nz * M = %ld, or nsel * nts >= 2^28) exceeds the capacity of one operand row (%ld doubles; "
               "GPCSD_MAX_GEMM_LD_KMAJOR)", who, M, nts, (long)nz * M, (long)GPCSD_MAX_GEMM_LD_KMAJOR);
}
static void plv_check(const char *who, int nz, int nsel, int R, int S) {
    GP_REQUIRE(nz > 0 && nsel > 0 && R > 0 && S > 0, -3, "%s: bad arguments", who);
    const long T = ((long)nz + 63) / 64;
    GP_REQUIRE((long)R * S < GPCSD_MAX_GEMM_LD_KMAJOR && nz < (1 << 21) && (double)T * (T + 1) / 2 * nsel * S < 2147483648.0, GPCSD_ERR_CAPACITY,
               "%s: R * S = %ld exceeds the capacity of one operand row (%ld doubles; GPCSD_MAX_GEMM_LD_KMAJOR), or nz = %d, nsel = %d, "
               "S = %d give too many tiles", who, (long)R * S, (long)GPCSD_MAX_GEMM_LD_KMAJOR, nz, nsel, S);
}

extern "C" int gpcsd_analytic(gpcsd_ctx *c, const double *x, int nz, int nts, long M, const double *A_re, const double *A_im, int nsel,
                              double *phase, double *amp, double *u_re, double *u_im) {
    GP_API_BEGIN(c)
    GP_REQUIRE(x && A_re && A_im, -3, "analytic: bad arguments");
    analytic_check("analytic", nz, nts, M, nsel);
    const size_t nin = (size_t)nz * nts * M, nout = (size_t)nz * nsel * M;
    AnalyticDesc d;
    d.X = c->upload<double>("op_in0", x, nin);
    d.Are = c->upload<double>("op_in1", A_re, (size_t)nsel * nts);
    d.Aim = c->upload<double>("op_in2", A_im, (size_t)nsel * nts);
    d.nz = nz; d.nts = nts; d.M = M; d.nsel = nsel;
    double *const host[4] = {phase, amp, u_re, u_im};
    double **const dev[4] = {&d.phase, &d.amp, &d.ure, &d.uim};
    int nwant = 0;
    for (int k = 0; k < 4; ++k) nwant += host[k] != nullptr;
    double *dO = c->buf<double>("op_out", nout * (size_t)std::max(nwant, 1));
    for (int k = 0, at = 0; k < 4; ++k)
        if (host[k]) *dev[k] = dO + nout * (size_t)at++;
    k_analytic(c, d, c->stream);
    for (int k = 0; k < 4; ++k)
        if (host[k]) c->download(host[k], *dev[k], nout * sizeof(double));
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_analytic_resident(gpcsd_ctx *c, const char *src_name, long src_offset, int nz, int nts, long M, const double *A_re,
                                       const double *A_im, int nsel, int want_mask) {
    GP_API_BEGIN(c)
    static const char *const out_name[4] = {"phase_out", "phase_amp", "phasor_re", "phasor_im"};
    GP_REQUIRE(src_name && A_re && A_im && src_offset >= 0 && want_mask > 0 && want_mask < 16, -3, "analytic_resident: bad arguments");
    analytic_check("analytic_resident", nz, nts, M, nsel);
    for (const char *n : out_name) GP_REQUIRE(strcmp(src_name, n) != 0, -3, "analytic_resident: '%s' is one of the call's outputs", n);
    auto it = c->bufs.find(src_name);
    GP_REQUIRE(it != c->bufs.end() && it->second.p, -2, "analytic_resident: no device buffer named '%s'", src_name);
    const size_t nin = (size_t)nz * nts * M, nout = (size_t)nz * nsel * M;
    GP_REQUIRE(((size_t)src_offset + nin) * sizeof(double) <= it->second.bytes, -3,
               "analytic_resident: '%s' holds %zu bytes, offset %ld + %zu doubles asked for", src_name, it->second.bytes, src_offset, nin);
    // a queued prediction that still owes its status produced the source: collected first, as gpcsd_fetch does
    if (int rc = drain_async(c)) return rc;
    AnalyticDesc d;
    d.X = static_cast<const double *>(it->second.p) + src_offset;
    d.Are = c->upload<double>("phase_A_re", A_re, (size_t)nsel * nts);
    d.Aim = c->upload<double>("phase_A_im", A_im, (size_t)nsel * nts);
    d.nz = nz; d.nts = nts; d.M = M; d.nsel = nsel;
    double **const dev[4] = {&d.phase, &d.amp, &d.ure, &d.uim};
    for (int k = 0; k < 4; ++k)
        if (want_mask & (1 << k)) *dev[k] = c->buf<double>(out_name[k], nout);
    c->phasor_shape[0] = c->phasor_shape[1] = c->phasor_shape[2] = 0;       // (until both halves of the phasors are in place)
    k_analytic(c, d, c->stream);
    c->sync();
    if ((want_mask & 12) == 12) {
        c->phasor_shape[0] = nz; c->phasor_shape[1] = nsel; c->phasor_shape[2] = M;
    }
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_plv(gpcsd_ctx *c, const double *u_re, const double *u_im, int nz, int nsel, int R, int S, double *c_re, double *c_im,
                         double *plv) {
    GP_API_BEGIN(c)
    GP_REQUIRE(u_re && u_im, -3, "plv: bad arguments");
    plv_check("plv", nz, nsel, R, S);
    const size_t nin = (size_t)nz * nsel * R * S, nout = (size_t)S * nsel * nz * nz;
    PlvDesc d;
    d.ure = c->upload<double>("op_in0", u_re, nin);
    d.uim = c->upload<double>("op_in1", u_im, nin);
    d.nz = nz; d.nsel = nsel; d.R = R; d.S = S;
    double *const host[3] = {c_re, c_im, plv};
    double **const dev[3] = {&d.cre, &d.cim, &d.plv};
    int nwant = 0;
    for (int k = 0; k < 3; ++k) nwant += host[k] != nullptr;
    double *dO = c->buf<double>("op_out", nout * (size_t)std::max(nwant, 1));
    for (int k = 0, at = 0; k < 3; ++k)
        if (host[k]) *dev[k] = dO + nout * (size_t)at++;
    k_plv(c, d, c->stream);
    for (int k = 0; k < 3; ++k)
        if (host[k]) c->download(host[k], *dev[k], nout * sizeof(double));
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_plv_resident(gpcsd_ctx *c, int nz, int nsel, int R, int S) {
    GP_API_BEGIN(c)
    plv_check("plv_resident", nz, nsel, R, S);
    GP_REQUIRE(c->phasor_shape[0] == nz && c->phasor_shape[1] == nsel && c->phasor_shape[2] == (long)R * S, -4,
               "plv_resident: no gpcsd_analytic_resident call has left unit phasors of shape (%d, %d, %d * %d) (found (%ld, %ld, %ld))", nz,
               nsel, R, S, c->phasor_shape[0], c->phasor_shape[1], c->phasor_shape[2]);
    const size_t nout = (size_t)S * nsel * nz * nz;
    PlvDesc d;
    d.ure = static_cast<const double *>(c->bufs["phasor_re"].p);
    d.uim = static_cast<const double *>(c->bufs["phasor_im"].p);
    d.nz = nz; d.nsel = nsel; d.R = R; d.S = S;
    d.cre = c->buf<double>("plv_re", nout);
    d.cim = c->buf<double>("plv_im", nout);
    d.plv = c->buf<double>("plv_abs", nout);
    k_plv(c, d, c->stream);
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

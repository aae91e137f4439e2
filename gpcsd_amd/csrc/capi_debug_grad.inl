// Part of capi.hip (included there, behind capi_grad.inl: hp_image and dbg_tri_idle are in scope) -- gpcsd_debug_grad_op: one
// launcher of grad.hip on the main stream with the caller's operands, host arrays in and out (include/gpcsd_hip.h has the table of
// operations).  Plumbing only: every operand's reach is checked against its length before anything is uploaded, the operands go up
// as given, the launcher is called with the arguments capi_grad.inl gives it, the results come down.
enum { DGO_TEMPORAL = 0, DGO_FROB_INNER, DGO_KGL, DGO_FROB_PAIR, DGO_FWDR, DGO_D_SUMS, DGO_BATCH_REDUCE, DGO_SIGLIST, DGO_ROWGROUP_SUMSQ,
       DGO_PER_TRIAL_QUAD, DGO_COUNT };

extern "C" int gpcsd_debug_grad_op(gpcsd_ctx *c, gpcsd_debug_grad_args *a) {
    GP_API_BEGIN(c)
    GP_REQUIRE(a, -3, "debug_grad_op: bad arguments");
    const int op = a->op, B = a->B;
    GP_REQUIRE(op >= 0 && op < DGO_COUNT, -3, "debug_grad_op: unknown op %d", op);
    GP_REQUIRE(B >= 1 && B <= 1024, -3, "debug_grad_op: %d sets (1 .. 1024)", B);
    const bool table = a->table != 0;
    const bool by_hp = op == DGO_TEMPORAL || op == DGO_KGL || op == DGO_FWDR;      // ops whose scalars can come by value
    GP_REQUIRE(by_hp || !table, -3, "debug_grad_op: op %d takes no table", op);
    GP_REQUIRE(!by_hp || table || B == 1, -3, "debug_grad_op: %d sets by value (a table is needed)", B);
    const bool sets = by_hp || op == DGO_FROB_PAIR || op == DGO_D_SUMS || op == DGO_BATCH_REDUCE || op == DGO_SIGLIST;
    GP_REQUIRE(sets || B == 1, -3, "debug_grad_op: op %d has no sets", op);
    const long LIM = 1L << 31;                             // (sizes whose products stay far inside 64 bits)
    for (int k = 0; k < 4; ++k) GP_REQUIRE(a->n[k] >= 0 && a->l[k] >= 0 && a->l[k] < LIM, -3, "debug_grad_op: a negative or huge size");
    auto need_in = [&](int k, long len, const char *what) {
        GP_REQUIRE(a->in[k] && len >= 1 && a->nin[k] >= len, -3, "debug_grad_op: %s needs %ld doubles (got %ld, %s)", what, len,
                   a->nin[k], a->in[k] ? "non-null" : "null");
    };
    auto need_out = [&](int k, long len, const char *what) {
        GP_REQUIRE(a->out[k] && len >= 1 && a->nout[k] == len, -3, "debug_grad_op: %s must hold %ld doubles (got %ld, %s)", what, len,
                   a->nout[k], a->out[k] ? "non-null" : "null");
    };
    static const char *const IN_BUF[6] = {"dbg_grad_in0", "dbg_grad_in1", "dbg_grad_in2", "dbg_grad_in3", "dbg_grad_in4", "dbg_grad_in5"};
    static const char *const OUT_BUF[4] = {"dbg_grad_out0", "dbg_grad_out1", "dbg_grad_out2", "dbg_grad_out3"};
    auto up = [&](int k) { return (const double *)c->upload<double>(IN_BUF[k], a->in[k], (size_t)a->nin[k]); };
    // an output starts as zeros, so that what a launcher leaves unwritten between the sets' results reads the same every time
    auto outbuf = [&](int k) {
        double *d = c->buf<double>(OUT_BUF[k], (size_t)a->nout[k]);
        GP_HIP(hipMemsetAsync(d, 0, (size_t)a->nout[k] * sizeof(double), c->stream));
        return d;
    };
    auto down = [&](int k, const double *d) { c->download(a->out[k], d, (size_t)a->nout[k] * sizeof(double)); };
    // hyper-parameter sets: checked, then as a device table (grad_front's way) where asked for
    auto check_hp = [&](int count) {
        GP_REQUIRE(a->hp, -3, "debug_grad_op: no hyper-parameters");
        for (int b = 0; b < count; ++b) {
            const gpcsd_hparams &h = a->hp[b];
            GP_REQUIRE(h.n_temporal >= 1 && h.n_temporal <= GPCSD_MAX_TEMPORAL, -3, "debug_grad_op: set %d has %d temporal components (1 .. %d)",
                       b, h.n_temporal, GPCSD_MAX_TEMPORAL);
            GP_REQUIRE(h.n_temporal <= a->hp[0].n_temporal, -3, "debug_grad_op: set %d has more temporal components than set 0", b);
            for (int i = 0; i < h.n_temporal; ++i)
                GP_REQUIRE(temporal_kind_on_device(h.kind[i]), -3, "debug_grad_op: set %d, component %d: kind %d",
                           b, i, h.kind[i]);
            GP_REQUIRE(h.sig2n, -3, "debug_grad_op: set %d has no noise variance", b);
        }
    };
    auto upload_tab = [&]() {
        std::vector<HpDev> himg(B);
        for (int b = 0; b < B; ++b) himg[b] = hp_image(&a->hp[b]);
        return (const HpDev *)c->upload<HpDev>("dbg_grad_tab", himg.data(), B);
    };
    const long s_out = a->l[3];
    const int nb_sets = by_hp && !table ? 1 : B;
    auto need_s_out = [&](long per_set) {
        GP_REQUIRE(s_out >= per_set, -3, "debug_grad_op: outputs %ld apart for %ld values per set", s_out, per_set);
        need_out(0, (long)nb_sets * s_out, "out");
    };

    switch (op) {
    case DGO_TEMPORAL: {
        const long nt = a->n[0];
        GP_REQUIRE(nt >= 1 && nt <= 46340, -3, "debug_grad_op: nt = %ld", nt);
        check_hp(nb_sets);
        need_in(0, nb_sets * nt * nt, "Gt");
        need_in(1, nt, "t");
        need_s_out(2L * a->hp[0].n_temporal);
        if (int rc = dbg_tri_idle(c)) return rc;           // (the launchers' scratch is the gradient evaluation's)
        const double *Gt = up(0), *t = up(1);
        double *o = outbuf(0);
        if (table) k_temporal_grad(c, &a->hp[0], Gt, t, (int)nt, o, c->stream, upload_tab(), B, s_out);
        else k_temporal_grad(c, &a->hp[0], Gt, t, (int)nt, o, c->stream);
        down(0, o);
        break;
    }
    case DGO_FROB_INNER: {
        const long n2 = a->l[0], nm = a->n[0];
        GP_REQUIRE(n2 >= 1 && nm >= 1 && nm <= 2 * GPCSD_MAX_TEMPORAL, -3, "debug_grad_op: frob_inner of %ld elements, %ld matrices", n2, nm);
        need_in(0, n2, "Gt");
        need_in(1, nm * n2, "dK");
        need_out(0, nm, "out");
        if (int rc = dbg_tri_idle(c)) return rc;
        const double *Gt = up(0), *dK = up(1);
        double *o = outbuf(0);
        k_frob_inner(c, Gt, dK, n2, (int)nm, o, c->stream);
        down(0, o);
        break;
    }
    case DGO_KGL: {
        const long G = a->n[0], ngl2 = a->n[1];
        GP_REQUIRE(G >= 1 && G <= 46340 && (ngl2 == 0 || G % ngl2 == 0), -3, "debug_grad_op: kgl_grad with G = %ld, ngl2 = %ld", G, ngl2);
        if (table) check_hp(B);
        need_in(0, nb_sets * G * G, "M");
        need_in(1, nb_sets * G * G, "Kgl");
        need_in(2, ngl2 > 0 ? G / ngl2 : G, "gx1");
        if (ngl2 > 0) need_in(3, ngl2, "gx2");
        need_s_out(ngl2 > 0 ? 2 : 1);
        if (int rc = dbg_tri_idle(c)) return rc;
        const double *M = up(0), *Kgl = up(1), *gx1 = up(2), *gx2 = ngl2 > 0 ? up(3) : nullptr;
        double *o = outbuf(0);
        if (table) k_kgl_grad(c, M, Kgl, gx1, gx2, (int)G, (int)ngl2, 0.0, 0.0, o, c->stream, upload_tab(), B, s_out);
        else k_kgl_grad(c, M, Kgl, gx1, gx2, (int)G, (int)ngl2, a->s[0], a->s[1], o, c->stream);
        down(0, o);
        break;
    }
    case DGO_FROB_PAIR: {
        const long n = a->l[0];
        GP_REQUIRE(n >= 1, -3, "debug_grad_op: frob_pair of %ld elements", n);
        need_in(0, B * n, "P");
        need_in(1, B * n, "T1");
        need_in(2, B * n, "T2");
        need_s_out(2);
        if (int rc = dbg_tri_idle(c)) return rc;
        const double *P = up(0), *T1 = up(1), *T2 = up(2);
        double *o = outbuf(0);
        k_frob_pair(c, P, T1, T2, n, o, c->stream, B, s_out);
        down(0, o);
        break;
    }
    case DGO_FWDR: {
        const long nx = a->n[0], G = a->n[1], ngl2 = a->n[2];
        GP_REQUIRE(nx >= 1 && G >= 1 && nx * G < LIM && (ngl2 == 0 || G % ngl2 == 0), -3,
                   "debug_grad_op: fwdR_grad with nx = %ld, G = %ld, ngl2 = %ld", nx, G, ngl2);
        if (table) check_hp(B);
        need_in(0, nb_sets * nx * G, "S");
        need_in(1, ngl2 > 0 ? 2 * nx : nx, "x");
        need_in(2, ngl2 > 0 ? G / ngl2 : G, "gx1");
        need_in(3, ngl2 > 0 ? G / ngl2 : G, "gw1");
        if (ngl2 > 0) {
            need_in(4, ngl2, "gx2");
            need_in(5, ngl2, "gw2");
        }
        need_s_out(1);
        if (int rc = dbg_tri_idle(c)) return rc;
        const double *S = up(0), *x = up(1), *gx1 = up(2), *gw1 = up(3), *gx2 = ngl2 > 0 ? up(4) : nullptr, *gw2 = ngl2 > 0 ? up(5) : nullptr;
        double *o = outbuf(0);
        if (table) k_fwdR_grad(c, S, x, (int)nx, gx1, gw1, gx2, gw2, (int)G, (int)ngl2, 0.0, 0.0, o, c->stream, upload_tab(), B, s_out);
        else k_fwdR_grad(c, S, x, (int)nx, gx1, gw1, gx2, gw2, (int)G, (int)ngl2, a->s[0], a->s[1], o, c->stream);
        down(0, o);
        break;
    }
    case DGO_D_SUMS: {
        const long nx = a->n[0], nt = a->n[1];
        GP_REQUIRE(nx >= 1 && nt >= 1 && nx <= 65535 && nx * nt < LIM, -3, "debug_grad_op: D_sums with nx = %ld, nt = %ld", nx, nt);
        need_in(0, B * nx * nt, "D");
        need_in(1, B * nx, "es");
        need_in(2, B * nt, "et");
        need_out(0, B * nx, "a");
        need_out(1, B * nt, "b");
        GP_REQUIRE(s_out >= 1, -3, "debug_grad_op: outputs %ld apart", s_out);
        need_out(2, B * s_out, "sum 1/D");
        need_out(3, B * nx, "row sums of 1/D");
        if (int rc = dbg_tri_idle(c)) return rc;
        const double *D = up(0), *es = up(1), *et = up(2);
        double *da = outbuf(0), *db = outbuf(1), *ds = outbuf(2);
        k_D_sums(c, D, es, et, (int)nx, (int)nt, da, db, ds, c->stream, B, s_out);
        down(0, da);
        down(1, db);
        down(2, ds);
        down(3, c->buf<double>("grad_s1row", (size_t)nx * B));
        break;
    }
    case DGO_BATCH_REDUCE: {
        const long nb = a->n[0], n = a->n[1], stride = a->l[0], s_in = a->l[1], s_dvec = a->l[2];
        GP_REQUIRE(nb >= 1 && n >= 1 && n <= 46340 && stride >= n * n, -3, "debug_grad_op: batch_reduce of %ld terms of order %ld, %ld apart",
                   nb, n, stride);
        need_in(0, (B - 1) * s_in + (nb - 1) * stride + n * n, "in");
        need_in(1, (B - 1) * s_dvec + n, "dvec");
        need_s_out(n * n);
        if (int rc = dbg_tri_idle(c)) return rc;
        const double *in = up(0), *dvec = up(1);
        double *o = outbuf(0);
        k_batch_reduce(c, in, (int)nb, stride, (int)n, a->s[0], dvec, a->s[1], o, c->stream, B, s_in, s_dvec, s_out);
        down(0, o);
        break;
    }
    case DGO_SIGLIST: {
        const long nx = a->n[0];
        GP_REQUIRE(nx >= 1 && nx <= 46340, -3, "debug_grad_op: siglist_eigvec_term with nx = %ld", nx);
        need_in(0, B * nx * nx, "Ghs");
        need_in(1, B * nx * nx, "Ssum");
        need_in(2, B * nx, "es");
        need_in(3, B * nx, "sig");
        need_out(0, B * nx * nx, "Ghs");
        if (int rc = dbg_tri_idle(c)) return rc;
        double *Ghs = c->upload<double>(IN_BUF[0], a->in[0], (size_t)a->nout[0]);
        const double *Ssum = up(1), *es = up(2), *sig = up(3);
        k_siglist_eigvec_term(c, Ghs, Ssum, es, sig, (int)nx, a->s[0], c->stream, B);
        down(0, Ghs);
        break;
    }
    case DGO_ROWGROUP_SUMSQ: {
        const long nrows = a->n[0], rowlen = a->l[0];
        GP_REQUIRE(nrows >= 1 && rowlen >= 1, -3, "debug_grad_op: rowgroup_sumsq of %ld rows of %ld", nrows, rowlen);
        need_in(0, nrows * rowlen, "B");
        need_out(0, nrows, "out");
        if (int rc = dbg_tri_idle(c)) return rc;
        const double *Bm = up(0);
        double *o = outbuf(0);
        k_rowgroup_sumsq(c, Bm, (int)nrows, rowlen, o, c->stream);
        down(0, o);
        break;
    }
    case DGO_PER_TRIAL_QUAD: {
        const long nx = a->n[0], nb = a->n[1], nt = a->n[2];
        GP_REQUIRE(nx >= 1 && nb >= 1 && nt >= 1 && nx * nt < LIM && nx * nb * nt < (1L << 40), -3,
                   "debug_grad_op: per_trial_quad with nx = %ld, nb = %ld, nt = %ld", nx, nb, nt);
        need_in(0, nx * nb * nt, "alpha");
        need_in(1, nx * nt, "D");
        need_out(0, nb, "out");
        if (int rc = dbg_tri_idle(c)) return rc;
        const double *al = up(0), *D = up(1);
        double *o = outbuf(0);
        k_per_trial_quad(c, al, D, (int)nx, (int)nb, (int)nt, o, c->stream);
        down(0, o);
        break;
    }
    }
    c->sync();
    return 0;
    GP_API_END(c)
}

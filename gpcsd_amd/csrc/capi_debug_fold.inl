// Part of capi.hip (included there, behind capi_debug_grad.inl: orbit_tables, temporal_fill, spatial_fill, hp_image and dbg_tri_idle
// are in scope) -- gpcsd_debug_fold_op: one launcher of the folded-basis / relayout family (gram.hip, eigh.hip) on the main stream
// with the caller's operands, host arrays in and out (include/gpcsd_hip.h has the table of operations).  Plumbing only: an orbit
// table is built from the caller's involution by find_symmetry's own routine, every operand's reach is checked against its length
// before anything is uploaded, every output starts as the caller's fill pattern and comes back whole.
enum { DFO_SWAP = 0, DFO_SWAP_SUM, DFO_FOLD_RECT, DFO_UNFOLD_MAT, DFO_FOLD_LFP, DFO_UNFOLD_SWAP_SUM, DFO_TEMPORAL_FILL, DFO_PSD_FILL,
       DFO_COUNT };

extern "C" int gpcsd_debug_fold_op(gpcsd_ctx *c, gpcsd_debug_fold_args *a) {
    GP_API_BEGIN(c)
    GP_REQUIRE(a, -3, "debug_fold_op: bad arguments");
    const int op = a->op, B = a->B;
    GP_REQUIRE(op >= 0 && op < DFO_COUNT, -3, "debug_fold_op: unknown op %d", op);
    GP_REQUIRE(B >= 1 && B <= 64, -3, "debug_fold_op: %d sets (1 .. 64)", B);
    const bool table = a->table != 0, with_list = a->list != 0;
    const bool fill_op = op == DFO_TEMPORAL_FILL || op == DFO_PSD_FILL;
    GP_REQUIRE(fill_op || !table, -3, "debug_fold_op: op %d takes no table", op);
    GP_REQUIRE(fill_op || op == DFO_UNFOLD_MAT || B == 1, -3, "debug_fold_op: op %d has no sets", op);
    GP_REQUIRE(!fill_op || table || B <= 2, -3, "debug_fold_op: %d sets by value (1 or 2; a table is needed)", B);
    const long LIM = 1L << 31;                             // (sizes whose products stay far inside 64 bits)
    for (int k = 0; k < 4; ++k)
        GP_REQUIRE(a->n[k] >= 0 && a->n[k] <= 65535 && a->l[k] >= 0 && a->l[k] < LIM, -3, "debug_fold_op: a negative or huge size");
    for (int k = 0; k < 2; ++k) GP_REQUIRE(a->nin[k] >= 0 && a->nin[k] < LIM, -3, "debug_fold_op: a negative or huge input length");
    for (int k = 0; k < 5; ++k) GP_REQUIRE(a->nout[k] >= 0 && a->nout[k] < LIM, -3, "debug_fold_op: a negative or huge output length");
    auto need_in = [&](int k, long len, const char *what) {
        GP_REQUIRE(a->in[k] && len >= 1 && a->nin[k] >= len, -3, "debug_fold_op: %s needs %ld doubles (got %ld, %s)", what, len, a->nin[k],
                   a->in[k] ? "non-null" : "null");
    };
    // (an output may be longer than its launcher's reach, and its reach may be zero -- an empty antisymmetric block --: what lies
    // beyond comes back as the fill pattern)
    auto need_out = [&](int k, long len, const char *what) {
        GP_REQUIRE(a->out[k] && a->nout[k] >= 1 && a->nout[k] >= len, -3, "debug_fold_op: %s must hold at least %ld doubles (got %ld, %s)",
                   what, std::max(len, 1L), a->nout[k], a->out[k] ? "non-null" : "null");
    };
    // an involution -> its orbit tables (find_symmetry's rule; the identity, which find_symmetry refuses, is identity_sym's table)
    std::vector<int> tbl[2];
    int sym_n[2] = {0, 0}, sym_na[2] = {0, 0};
    auto check_perm = [&](int k, const char *what) {
        const int n = a->nperm[k];
        GP_REQUIRE(a->perm[k] && n >= 1 && n <= 4096, -3, "debug_fold_op: the %s involution has %d points (1 .. 4096, %s)", what, n,
                   a->perm[k] ? "non-null" : "null");
        std::vector<int> perm(a->perm[k], a->perm[k] + n);
        for (int i = 0; i < n; ++i)
            GP_REQUIRE(perm[i] >= 0 && perm[i] < n && perm[perm[i]] == i, -3, "debug_fold_op: the %s permutation is no involution at %d",
                       what, i);
        sym_na[k] = orbit_tables(perm, tbl[k]);
        sym_n[k] = n;
    };
    static const char *const SYM_BUF[2] = {"dbg_fold_sym0", "dbg_fold_sym1"};
    auto upload_sym = [&](int k) {
        const int n = sym_n[k], ns = n - sym_na[k];
        const int *d = c->upload<int>(SYM_BUF[k], tbl[k].data(), tbl[k].size());
        SymDev sy;
        sy.ns = ns; sy.na = sym_na[k];
        sy.rep_i = d; sy.rep_j = d + ns; sy.orb = d + 2 * ns; sy.sgn = d + 2 * ns + n;
        return sy;
    };
    static const char *const IN_BUF[2] = {"dbg_fold_in0", "dbg_fold_in1"};
    static const char *const OUT_BUF[2] = {"dbg_fold_out0", "dbg_fold_out1"};
    auto up = [&](int k) { return (const double *)c->upload<double>(IN_BUF[k], a->in[k], (size_t)a->nin[k]); };
    auto outbuf = [&](int k) {
        double *d = c->buf<double>(OUT_BUF[k], (size_t)a->nout[k]);
        k_fill(c, d, a->nout[k], a->fill, c->stream);
        return d;
    };
    auto down = [&](int k, const double *d) { c->download(a->out[k], d, (size_t)a->nout[k] * sizeof(double)); };

    switch (op) {
    case DFO_SWAP: {
        const long n0 = a->n[0], n1 = a->n[1], n2 = a->n[2], tot = n0 * n1 * n2;
        GP_REQUIRE(n0 >= 1 && n1 >= 1 && n2 >= 1 && tot < LIM, -3, "debug_fold_op: swap_last2 of (%ld, %ld, %ld)", n0, n1, n2);
        need_in(0, tot, "in");
        need_out(0, tot, "out");
        if (int rc = dbg_tri_idle(c)) return rc;
        const double *in = up(0);
        double *o = outbuf(0);
        k_swap_last2(c, in, o, (int)n0, (int)n1, (int)n2, c->stream);
        down(0, o);
        break;
    }
    case DFO_SWAP_SUM: {
        const long n0 = a->n[0], n1 = a->n[1], n2 = a->n[2], C = a->n[3], tot = n0 * n1 * n2, ls = a->l[0];
        GP_REQUIRE(n0 >= 1 && n1 >= 1 && n2 >= 1 && tot * GPCSD_MAX_TEMPORAL < LIM && C >= 1 && C <= GPCSD_MAX_TEMPORAL, -3,
                   "debug_fold_op: swap_last2_sum of (%ld, %ld, %ld), %ld components", n0, n1, n2, C);
        need_in(0, tot * C, "in");
        need_out(0, tot, "sum");
        if (with_list) {
            GP_REQUIRE(ls >= tot && (C - 1) * ls + tot < LIM, -3, "debug_fold_op: lists %ld apart for %ld values each", ls, tot);
            need_out(1, (C - 1) * ls + tot, "list");
        }
        if (int rc = dbg_tri_idle(c)) return rc;
        const double *in = up(0);
        double *sum = outbuf(0), *list = with_list ? outbuf(1) : nullptr;
        k_swap_last2_sum(c, in, (int)C, list, ls, sum, (int)n0, (int)n1, (int)n2, c->stream);
        down(0, sum);
        if (with_list) down(1, list);
        break;
    }
    case DFO_FOLD_RECT: {
        check_perm(0, "row");
        check_perm(1, "column");
        const long nr = sym_n[0], nc = sym_n[1], ldk = a->l[0];
        const long rns = nr - sym_na[0], cns = nc - sym_na[1];
        GP_REQUIRE(ldk >= nc && (nr - 1) * ldk + nc < LIM, -3, "debug_fold_op: rows %ld apart for %ld columns", ldk, nc);
        need_in(0, (nr - 1) * ldk + nc, "K");
        need_out(0, rns * cns, "out_ss");
        need_out(1, (long)sym_na[0] * sym_na[1], "out_aa");
        if (int rc = dbg_tri_idle(c)) return rc;
        const SymDev rs = upload_sym(0), cs = upload_sym(1);
        const double *K = up(0);
        double *oss = outbuf(0), *oaa = outbuf(1);
        k_sym_fold_rect(c, K, ldk, rs, cs, oss, oaa, c->stream);
        down(0, oss);
        down(1, oaa);
        break;
    }
    case DFO_UNFOLD_MAT: {
        check_perm(0, "matrix");
        const long n = sym_n[0], na = sym_na[0], ns = n - na, blk = ns * ns + na * na, s_in = a->l[0];
        GP_REQUIRE(s_in >= blk && (B - 1) * s_in + blk < LIM, -3, "debug_fold_op: folded sets %ld apart for %ld values each", s_in, blk);
        need_in(0, (B - 1) * s_in + blk, "Gf");
        need_out(0, B * n * n, "out");
        if (int rc = dbg_tri_idle(c)) return rc;
        const SymDev sy = upload_sym(0);
        const double *Gf = up(0);
        double *o = outbuf(0);
        k_sym_unfold_mat(c, Gf, s_in, sy, (int)n, o, c->stream, B);
        down(0, o);
        break;
    }
    case DFO_FOLD_LFP: {
        check_perm(0, "spatial");
        check_perm(1, "temporal");
        const long nx = sym_n[0], nt = sym_n[1], R = a->n[0], tot = nx * R * nt;
        GP_REQUIRE(R >= 1 && tot < LIM, -3, "debug_fold_op: fold_lfp of (%ld, %ld, %ld)", nx, R, nt);
        need_in(0, tot, "Y");
        need_out(0, tot, "out");
        if (int rc = dbg_tri_idle(c)) return rc;
        const SymDev ss = upload_sym(0), st = upload_sym(1);
        const double *Y = up(0);
        double *o = outbuf(0);
        k_fold_lfp(c, Y, (int)nx, (int)R, (int)nt, ss, st, o, c->stream);
        down(0, o);
        break;
    }
    case DFO_UNFOLD_SWAP_SUM: {
        check_perm(0, "site");
        check_perm(1, "time");
        const long nz = sym_n[0], nt = sym_n[1], tna = sym_na[1], tns = nt - tna, R = a->n[0], C = a->n[1], ls = a->l[0];
        const long tot = nz * nt * R;
        GP_REQUIRE(R >= 1 && C >= 1 && C <= GPCSD_MAX_TEMPORAL && tot * GPCSD_MAX_TEMPORAL < LIM, -3,
                   "debug_fold_op: unfold_swap_sum of (%ld, %ld, %ld), %ld components", nz, nt, R, C);
        // the launcher's defaults, formed here as it forms them (0 = default): the reach below is that of the effective layout
        const long nsP = a->n[2] > 0 ? a->n[2] : tns, naP = a->n[3] > 0 ? a->n[3] : tna;
        const long ldin = a->l[1] > 0 ? a->l[1] : C * (nsP + naP);
        GP_REQUIRE(nsP >= tns && naP >= tna && ldin >= C * (nsP + naP) && (nz * R - 1) * ldin + C * (nsP + naP) < LIM, -3,
                   "debug_fold_op: column blocks of %ld / %ld for %ld / %ld orbits, rows %ld apart", nsP, naP, tns, tna, ldin);
        const long last_col = tna > 0 ? C * nsP + (C - 1) * naP + tna : (C - 1) * nsP + tns;
        need_in(0, (nz * R - 1) * ldin + last_col, "in");
        need_out(0, tot, "sum");
        if (with_list) {
            GP_REQUIRE(ls >= tot && (C - 1) * ls + tot < LIM, -3, "debug_fold_op: lists %ld apart for %ld values each", ls, tot);
            need_out(1, (C - 1) * ls + tot, "list");
        }
        if (int rc = dbg_tri_idle(c)) return rc;
        const SymDev sz = upload_sym(0), st = upload_sym(1);
        const double *in = up(0);
        double *sum = outbuf(0), *list = with_list ? outbuf(1) : nullptr;
        k_unfold_swap_sum(c, in, (int)C, list, ls, sum, (int)R, (int)nt, sz, st, c->stream, a->n[2], a->n[3], a->l[1]);
        down(0, sum);
        if (with_list) down(1, list);
        break;
    }
    case DFO_TEMPORAL_FILL:
    case DFO_PSD_FILL: {
        const bool temporal = op == DFO_TEMPORAL_FILL;
        check_perm(0, "grid");
        const long n = sym_n[0], na = sym_na[0], ns = n - na;
        GP_REQUIRE(na >= 1 && n <= GPCSD_MAX_EIG_N, -3, "debug_fold_op: a fill needs a pair (%ld points, %ld pairs)", n, na);
        const long sK = temporal ? 0 : a->l[0];
        if (temporal) {
            GP_REQUIRE(a->hp, -3, "debug_fold_op: no hyper-parameters");
            for (int b = 0; b < B; ++b) {
                const gpcsd_hparams &h = a->hp[b];
                GP_REQUIRE(h.n_temporal >= 1 && h.n_temporal <= GPCSD_MAX_TEMPORAL, -3, "debug_fold_op: set %d has %d temporal components (1 .. %d)",
                           b, h.n_temporal, GPCSD_MAX_TEMPORAL);
                for (int i = 0; i < h.n_temporal; ++i)
                    GP_REQUIRE(temporal_kind_on_device(h.kind[i]), -3, "debug_fold_op: set %d, component %d: kind %d", b, i, h.kind[i]);
                GP_REQUIRE(h.sig2n, -3, "debug_fold_op: set %d has no noise variance", b);
            }
            need_in(0, n, "t");
        } else {
            GP_REQUIRE(sK == 0 || sK >= n * n, -3, "debug_fold_op: sources %ld apart for %ld values each", sK, n * n);
            GP_REQUIRE(!table || a->hp, -3, "debug_fold_op: no hyper-parameters");
            for (int b = 0; table && b < B; ++b) {
                const gpcsd_hparams &h = a->hp[b];
                GP_REQUIRE(h.n_temporal >= 1 && h.n_temporal <= GPCSD_MAX_TEMPORAL && h.sig2n, -3,
                           "debug_fold_op: set %d is no hyper-parameter set", b);
            }
            need_in(0, (B - 1) * sK + n * n, "K");
        }
        // per set: both blocks; the reflector storage of both classes and one word more each; tau's n + 66 words and one more each
        const long nv[2] = {(ns + 64) * ns + 1, (na + 64) * na + 1}, ntau[2] = {ns + 67, na + 67};
        need_out(0, B * ns * ns, "A0s");
        need_out(1, B * na * na, "A0a");
        need_out(2, B * (nv[0] + nv[1]), "V");
        need_out(3, B * (ntau[0] + ntau[1]), "tau");
        need_out(4, 2L * B, "amax");
        GP_REQUIRE(a->status && a->nstatus >= B, -3, "debug_fold_op: status must hold %d words", B);
        // an idle context, and nothing of an earlier call that lives in these arenas is reused afterwards
        if (int rc = dbg_tri_idle(c)) return rc;
        if (c->stream5) GP_HIP(hipStreamSynchronize(c->stream5));
        pair_prefetch_drop(c);
        c->decomp_gen[0] = c->decomp_gen[1] = -1;
        const SymDev sy = upload_sym(0);
        const double *in = up(0);
        int *st = c->buf<int>("dbg_fold_status", (size_t)a->nstatus);
        GP_HIP(hipMemsetAsync(st, 0, (size_t)a->nstatus * sizeof(int), c->stream));
        const char *const *tg = eigh_fold_tags(c, temporal ? 1 : 0);
        const EigArenaView av[2] = {eigh_arena_view(c, tg[0], (int)ns, B), eigh_arena_view(c, tg[1], (int)na, B)};
        const long nsq[2] = {ns * ns, na * na};
        for (int h = 0; h < 2; ++h)
            for (int b = 0; b < B; ++b) {
                const long o = b * av[h].blk;
                k_fill(c, av[h].A0 + o, nsq[h], a->fill, c->stream);
                k_fill(c, av[h].V + o, nv[h], a->fill, c->stream);
                k_fill(c, av[h].tau + o, ntau[h], a->fill, c->stream);
                k_fill(c, av[h].amax + o, 1, a->fill, c->stream);
            }
        const HpDev *tab = nullptr;
        bool nonneg = true;
        if (table) {
            std::vector<HpDev> himg(B);
            for (int b = 0; b < B; ++b) {
                himg[b] = hp_image(&a->hp[b]);
                nonneg = nonneg && himg[b].jitter >= 0.0;
                for (int i = 0; i < himg[b].ncomp; ++i) nonneg = nonneg && himg[b].sigma2_t[i] >= 0.0;
            }
            tab = c->upload<HpDev>("dbg_fold_tab", himg.data(), B);
        }
        if (temporal) {
            if (table) k_temporal_fold_fill_tab(c, tab, B, in, (int)n, sy, av[0], av[1], st, 1, c->stream, nonneg);
            else {
                const gpcsd_hparams *hps[2] = {&a->hp[0], &a->hp[B - 1]};
                temporal_fill(c, hps, B, in, (int)n, sy, st, 1, c->stream);
            }
        } else {
            if (table) k_psd_fold_fill(c, in, (int)n, sK, B, nullptr, sy, av[0], av[1], st, 1, c->stream, tab, nonneg);
            else spatial_fill(c, in, (int)n, sK, B, a->s, sy, st, 1, c->stream);
        }
        double *o0 = a->out[0], *o1 = a->out[1], *o2 = a->out[2], *o3 = a->out[3], *o4 = a->out[4];
        // (an output longer than the sets' results: the rest is the fill pattern, as for the other operations)
        auto pattern = [&](int k, long from) {
            for (long i = from; i < a->nout[k]; ++i) a->out[k][i] = a->fill;
        };
        pattern(0, B * nsq[0]);
        pattern(1, B * nsq[1]);
        pattern(2, B * (nv[0] + nv[1]));
        pattern(3, B * (ntau[0] + ntau[1]));
        pattern(4, 2L * B);
        for (int b = 0; b < B; ++b) {
            const long os = b * av[0].blk, oa = b * av[1].blk;
            c->download(o0 + b * nsq[0], av[0].A0 + os, (size_t)nsq[0] * sizeof(double));
            c->download(o1 + b * nsq[1], av[1].A0 + oa, (size_t)nsq[1] * sizeof(double));
            c->download(o2 + b * (nv[0] + nv[1]), av[0].V + os, (size_t)nv[0] * sizeof(double));
            c->download(o2 + b * (nv[0] + nv[1]) + nv[0], av[1].V + oa, (size_t)nv[1] * sizeof(double));
            c->download(o3 + b * (ntau[0] + ntau[1]), av[0].tau + os, (size_t)ntau[0] * sizeof(double));
            c->download(o3 + b * (ntau[0] + ntau[1]) + ntau[0], av[1].tau + oa, (size_t)ntau[1] * sizeof(double));
            c->download(o4 + 2 * b, av[0].amax + os, sizeof(double));
            c->download(o4 + 2 * b + 1, av[1].amax + oa, sizeof(double));
        }
        c->download(a->status, st, (size_t)a->nstatus * sizeof(int));
        c->sync();
        // the arenas hold no decomposition's input any more: what the fills announced about them goes with it
        c->arena_psd[tg[0]] = c->arena_psd[tg[1]] = false;
        break;
    }
    }
    c->sync();
    return 0;
    GP_API_END(c)
}

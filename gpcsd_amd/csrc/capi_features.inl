// Part of capi.hip (included there: one translation unit, so the file-local helpers of capi.hip, capi_posterior.inl and capi_sample.inl
// are in scope) -- region features of a field (features.hip): of a host or resident field (gpcsd_region_features) and of posterior
// draws chunk by chunk inside the sampler (gpcsd_sample_features), where nothing but the answer grows with the number of draws.

// The label map as the lists features.hip reads (FeatPlan), on the host: every region's points in row-major order, cut into slices
struct FeatLists {
    std::vector<int> idx, slice_beg, slice_cnt, reg_slice;
};
// (everything a call can refuse about its regions, before anything is read on the device; P: columns of the output)
static void feat_check(const char *who, const int *labels, long npts, int J, long P) {
    GP_REQUIRE(labels != nullptr, -3, "%s: bad arguments", who);
    GP_REQUIRE(J >= 1, -3, "%s: J=%d regions; at least 1", who, J);
    GP_REQUIRE(J <= GPCSD_MAX_REGIONS && npts < (1L << 31) && (double)J * GPCSD_NFEAT * (double)P < 2147483648.0 && P < 64L * 65535,
               GPCSD_ERR_CAPACITY, "%s: J = %d regions (at most %d; GPCSD_MAX_REGIONS), %ld points (below 2^31) or J * %d * %ld feature values "
               "(below 2^31) exceed the capacity", who, J, GPCSD_MAX_REGIONS, npts, GPCSD_NFEAT, P);
    for (long k = 0; k < npts; ++k)
        GP_REQUIRE(labels[k] >= 0 && labels[k] <= J, -3, "%s: label %d at point %ld is outside [0, %d]", who, labels[k], k, J);
}
static FeatLists feat_lists(const int *labels, long npts, int J) {
    FeatLists L;
    std::vector<int> first((size_t)J + 2, 0);                 // counting sort by label: stable, so row-major inside a region
    for (long k = 0; k < npts; ++k) ++first[(size_t)labels[k] + 1];
    first[1] = 0;                                             // (label 0, the background, is not listed)
    for (int j = 1; j <= J; ++j) first[(size_t)j + 1] += first[j];
    L.idx.resize((size_t)first[(size_t)J + 1]);
    std::vector<int> at(first.begin() + 1, first.end());
    for (long k = 0; k < npts; ++k)
        if (labels[k] > 0) L.idx[(size_t)at[(size_t)labels[k] - 1]++] = (int)k;
    L.reg_slice.push_back(0);
    for (int j = 1; j <= J; ++j) {
        for (int b = first[j]; b < first[(size_t)j + 1]; b += FEAT_SLICE) {
            L.slice_beg.push_back(b);
            L.slice_cnt.push_back(std::min(FEAT_SLICE, first[(size_t)j + 1] - b));
        }
        L.reg_slice.push_back((int)L.slice_beg.size());
    }
    return L;
}
// ... on the device, with the coordinates of every listed point (tau (nts) and zeta (nz, dim) on the device)
static FeatPlan feat_plan(gpcsd_ctx *c, const FeatLists &L, int J, int nts, const double *tau, const double *zeta, int dim) {
    FeatPlan pl;
    pl.J = J; pl.nslice = (int)L.slice_beg.size(); pl.npts = (int)L.idx.size();
    pl.idx = c->upload<int>("feat_idx", L.idx.data(), L.idx.size());
    pl.slice_beg = c->upload<int>("feat_slice_beg", L.slice_beg.data(), L.slice_beg.size());
    pl.slice_cnt = c->upload<int>("feat_slice_cnt", L.slice_cnt.data(), L.slice_cnt.size());
    pl.reg_slice = c->upload<int>("feat_reg_slice", L.reg_slice.data(), L.reg_slice.size());
    double *co = c->buf<double>("feat_coords", 3 * L.idx.size());
    pl.ptau = co; pl.pz0 = co + L.idx.size(); pl.pz1 = co + 2 * L.idx.size();
    k_feat_coords(c, pl.idx, pl.npts, nts, tau, zeta, dim, co, co + L.idx.size(), co + 2 * L.idx.size(), c->stream);
    return pl;
}

static void region_features_check(const char *who, int nz, int nts, long M, const int *labels, int J, const double *tau, const double *zeta,
                                  int dim, const double *mean, const double *isd, int R, int S) {
    GP_REQUIRE(nz > 0 && nts > 0 && M > 0 && tau && zeta && (dim == 1 || dim == 2), -3, "%s: bad arguments", who);
    GP_REQUIRE((mean == nullptr) == (isd == nullptr), -3, "%s: give both mean and isd, or neither", who);
    GP_REQUIRE(!mean || (R > 0 && S > 0 && (long)R * S == M), -3, "%s: with a mean the M = %ld columns are R * S = %d * %d", who, M, R, S);
    feat_check(who, labels, (long)nz * nts, J, M);
}
// the field at dF (nz, nts, M) on the device -> feat (J, GPCSD_NFEAT, M) at dfeat; everything else from the host
static void region_features_run(gpcsd_ctx *c, const double *dF, int nz, int nts, long M, const int *labels, int J, const double *tau,
                                const double *zeta, int dim, const double *mean, const double *isd, int R, int S, double *dfeat) {
    const FeatLists L = feat_lists(labels, (long)nz * nts, J);
    const double *dtau = c->upload<double>("feat_tau", tau, (size_t)nts);
    const double *dzeta = c->upload<double>("feat_zeta", zeta, (size_t)nz * dim);
    const FeatPlan pl = feat_plan(c, L, J, nts, dtau, dzeta, dim);
    FeatDesc d;
    d.F = dF; d.ld = M; d.ncol = (int)M; d.col0 = 0; d.feat = dfeat; d.ldf = M;
    if (mean) {
        d.mean = c->upload<double>("feat_mean_in", mean, (size_t)nz * nts * R);
        d.isd = c->upload<double>("feat_isd_in", isd, (size_t)nz * nts);
        d.R = R; d.S = S;
    }
    d.part = c->buf<double>("feat_part", (size_t)std::max(pl.nslice, 1) * GPCSD_NFEAT * (size_t)M);
    k_region_features(c, pl, d, c->stream);
}

extern "C" int gpcsd_region_features(gpcsd_ctx *c, const double *x, int nz, int nts, long M, const int *labels, int J, const double *tau,
                                     const double *zeta, int dim, const double *mean, const double *isd, int R, int S, double *feat) {
    GP_API_BEGIN(c)
    GP_REQUIRE(x && feat, -3, "region_features: bad arguments");
    region_features_check("region_features", nz, nts, M, labels, J, tau, zeta, dim, mean, isd, R, S);
    const double *dF = c->upload<double>("op_in0", x, (size_t)nz * nts * M);
    double *dO = c->buf<double>("op_out", (size_t)J * GPCSD_NFEAT * M);
    region_features_run(c, dF, nz, nts, M, labels, J, tau, zeta, dim, mean, isd, R, S, dO);
    c->download(feat, dO, (size_t)J * GPCSD_NFEAT * M * sizeof(double));
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

extern "C" int gpcsd_region_features_resident(gpcsd_ctx *c, const char *src_name, long src_offset, int nz, int nts, long M, const int *labels,
                                              int J, const double *tau, const double *zeta, int dim, const double *mean, const double *isd,
                                              int R, int S) {
    GP_API_BEGIN(c)
    GP_REQUIRE(src_name && src_offset >= 0, -3, "region_features_resident: bad arguments");
    region_features_check("region_features_resident", nz, nts, M, labels, J, tau, zeta, dim, mean, isd, R, S);
    GP_REQUIRE(strcmp(src_name, "feat_out") != 0, -3, "region_features_resident: 'feat_out' is the call's output");
    auto it = c->bufs.find(src_name);
    GP_REQUIRE(it != c->bufs.end() && it->second.p, -2, "region_features_resident: no device buffer named '%s'", src_name);
    const size_t nin = (size_t)nz * nts * M;
    GP_REQUIRE(((size_t)src_offset + nin) * sizeof(double) <= it->second.bytes, -3,
               "region_features_resident: '%s' holds %zu bytes, offset %ld + %zu doubles asked for", src_name, it->second.bytes, src_offset, nin);
    // a queued prediction that still owes its status produced the source: collected first, as gpcsd_fetch does
    if (int rc = drain_async(c)) return rc;
    double *dO = c->buf<double>("feat_out", (size_t)J * GPCSD_NFEAT * M);
    region_features_run(c, static_cast<const double *>(c->bufs[src_name].p) + src_offset, nz, nts, M, labels, J, tau, zeta, dim, mean, isd, R,
                        S, dO);
    c->sync();
    if (c->prof_mode == 1) c->prof_collect();
    return 0;
    GP_API_END(c)
}

// The mean of gpcsd_predict_at and the variance of gpcsd_predict_var at the call's sites and times, through those calls' own
// internals, into buffers of this call: feat_mean_csd / feat_mean_lfp (nz, ntstar, R), feat_var_csd / feat_var_lfp (nz, ntstar), and
// feat_isd_csd / feat_isd_lfp = 1 / sqrt(var) where var > floor * max(var), 0 elsewhere.  pred_out_* and pred_var_* are not touched.
static int feature_band(gpcsd_ctx *c, const PredCall &q, double floor) {
    const int R = c->ntrials;
    const size_t out_elems = (size_t)q.nz * q.ntstar;
    {
        PostFront f;
        if (int rc = posterior_front(c, q, FRONT_DRAIN | FRONT_TRIALS, f)) return rc;
        double *S = c->buf<double>("pred_S", (size_t)q.nz * R * c->nt);
        for (int which = 1; which <= 2; ++which)
            if (q.type & which)
                pred_mean_tail(c, f, q, which, R, S, c->buf<double>(which == 1 ? "feat_mean_csd" : "feat_mean_lfp", out_elems * R), nullptr, 0);
        if (int rc = finish_call(c, f.e, nullptr, 0)) return rc;
    }
    if (int rc = predict_var_impl(c, q, "feat_var_")) return rc;
    double *vmax = c->buf<double>("feat_vmax", 1);
    for (int which = 1; which <= 2; ++which)
        if (q.type & which)
            k_feat_isd(c, c->buf<double>(which == 1 ? "feat_var_csd" : "feat_var_lfp", out_elems), (long)out_elems, floor, vmax,
                       c->buf<double>(which == 1 ? "feat_isd_csd" : "feat_isd_lfp", out_elems), c->stream);
    return 0;
}

// gpcsd_sample_posterior with the features of every chunk's draws reduced behind its combine pass, into columns [p0, p0 + np) of
// feat_csd / feat_lfp (J, GPCSD_NFEAT, R * nsamples).  tau = tstar, zeta = z.
static int sample_features_impl(gpcsd_ctx *c, const PredCall &q, int nsamples, unsigned long long seed, const double *normals_xi,
                                const double *normals_eps, const int *labels, int J, int with_band, double floor, int keep_draws) {
    const char *who = "sample_features";
    posterior_request(c, who, q, REQ_SITES);
    GP_REQUIRE(nsamples >= 1, -3, "%s: nsamples=%d must be at least 1", who, nsamples);
    GP_REQUIRE(!with_band || (floor >= 0.0 && floor < 1.0), -3, "%s: floor=%g must lie in [0, 1)", who, floor);
    const long P = (long)c->ntrials * nsamples;
    feat_check(who, labels, (long)q.nz * q.ntstar, J, std::max(P, 1L));
    posterior_request(c, who, q, REQ_HP | REQ_LFP | REQ_NO_HOST_KT | (with_band ? REQ_CAP_OUT_ROW | REQ_CAP_PC_ROW : 0u));
    const int dim = resident_geo(c).dim, R = c->ntrials, nz = q.nz, nts = q.ntstar;
    const FeatLists L = feat_lists(labels, (long)nz * nts, J);
    const size_t nslice = L.slice_beg.size();
    FeatPlan pl;
    double *feat[2] = {nullptr, nullptr};
    SampleSink sink;
    sink.keep_draws = keep_draws != 0;
    sink.per_extra = (size_t)nz * nts + nslice * GPCSD_NFEAT;
    sink.prelude = [&]() -> int {
        if (with_band)
            if (int rc = feature_band(c, q, floor)) return rc;
        const double *dtau = c->upload<double>("feat_tau", q.tstar, (size_t)nts);
        const double *dzeta = c->upload<double>("feat_zeta", q.z, (size_t)nz * dim);
        pl = feat_plan(c, L, J, nts, dtau, dzeta, dim);
        for (int w = 0; w < 2; ++w)
            if (q.type & (w + 1)) feat[w] = c->buf<double>(w ? "feat_lfp" : "feat_csd", (size_t)J * GPCSD_NFEAT * P);
        return 0;
    };
    sink.consume = [&](int which, const double *F, long ld, long p0, int np) {
        FeatDesc d;
        d.F = F; d.ld = ld; d.ncol = np; d.col0 = p0; d.feat = feat[which - 1]; d.ldf = P;
        if (with_band) {
            d.mean = static_cast<const double *>(c->bufs[which == 1 ? "feat_mean_csd" : "feat_mean_lfp"].p);
            d.isd = static_cast<const double *>(c->bufs[which == 1 ? "feat_isd_csd" : "feat_isd_lfp"].p);
            d.R = R; d.S = nsamples;
        }
        d.part = c->buf<double>("feat_part", std::max<size_t>(nslice, 1) * GPCSD_NFEAT * (size_t)np);
        k_region_features(c, pl, d, c->stream);
    };
    return sample_posterior_impl(c, q, nsamples, seed, normals_xi, normals_eps, &sink);
}

extern "C" int gpcsd_sample_features_resident(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar,
                                              int ntstar, int type, int nsamples, unsigned long long seed, const double *normals_xi,
                                              const double *normals_eps, const int *labels, int J, int with_band, double floor,
                                              int keep_draws) {
    GP_API_BEGIN(c)
    return sample_features_impl(c, pred_call(hp, z, nz, tstar, ntstar, type, false, false), nsamples, seed, normals_xi, normals_eps, labels, J,
                                with_band, floor, keep_draws);
    GP_API_END(c)
}

extern "C" int gpcsd_sample_features(gpcsd_ctx *c, const gpcsd_hparams *hp, const double *z, int nz, const double *tstar, int ntstar,
                                     int type, int nsamples, unsigned long long seed, const double *normals_xi, const double *normals_eps,
                                     const int *labels, int J, int with_band, double floor, int keep_draws, double *feat_csd,
                                     double *feat_lfp, double *csd, double *lfp) {
    GP_API_BEGIN(c)
    GP_REQUIRE(keep_draws || (!csd && !lfp), -3, "sample_features: draws asked for with keep_draws = 0");
    const int rc = sample_features_impl(c, pred_call(hp, z, nz, tstar, ntstar, type, false, false), nsamples, seed, normals_xi, normals_eps,
                                        labels, J, with_band, floor, keep_draws);
    if (rc < 0) return rc;
    const size_t P = (size_t)c->ntrials * nsamples, nfeat = (size_t)J * GPCSD_NFEAT * P, ndraw = (size_t)nz * ntstar * P;
    std::vector<HostOut> outs = {{(type & 1) ? feat_csd : nullptr, "feat_csd", nfeat}, {(type & 2) ? feat_lfp : nullptr, "feat_lfp", nfeat}};
    if (keep_draws) {
        outs.push_back({(type & 1) ? csd : nullptr, "post_sample_csd", ndraw});
        outs.push_back({(type & 2) ? lfp : nullptr, "post_sample_lfp", ndraw});
    }
    for (const HostOut &o : outs) {       // (a numerical failure, rc > 0, in front of the sampler leaves some of them unformed)
        auto it = c->bufs.find(o.name);
        if (o.host && it != c->bufs.end() && it->second.p) c->download(o.host, it->second.p, o.count * sizeof(double));
    }
    c->sync();
    return rc;
    GP_API_END(c)
}

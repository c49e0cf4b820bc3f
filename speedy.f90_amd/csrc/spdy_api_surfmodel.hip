// C ABI of the surface models (include/spdy.h, "surface models"): the slab land, sea and ice models of couple_sea_land and the
// column part of set_forcing, device-resident.  Kernels: csrc/spdy_surfmodel.hip; host tables: csrc/spdy_tables.cpp
// (SurfaceTables, surface_date_weights).
#include <cstring>

#include "spdy_plan.hpp"

using namespace spdy_detail;

namespace {
// member 0 of a field held per member (the base of its (nmem, il, ix) stack), the field itself where it is held once
double *field(const spdy_surface_model *m, int n) { return m->d_f + (size_t)spdy::surf_slot(n, m->nmem, 0) * m->ncol; }

int field_index(const char *name)
{
    static const char *const names[spdy::SM_NFIELDS] = {
        "fmask_l", "fmask_s", "alb0", "rhcapl", "cdland", "rhcaps", "rhcapi", "cdsea", "cdice",
        "stlcl_ob", "snowdcl_ob", "soilwcl_ob", "stl_lm", "stl_am", "snowd_am", "soilw_am",
        "sstcl_ob", "sicecl_ob", "ticecl_ob", "sstan_ob", "sst_om", "tice_om", "sice_om",
        "sst_am", "sstan_am", "sice_am", "tice_am", "ssti_om",
        "snowc", "alb_l", "alb_s", "albsfc", "corh"};
    for (int i = 0; i < spdy::SM_NFIELDS; ++i)
        if (!std::strcmp(name, names[i])) return i;
    return -1;
}
}  // namespace

extern "C" {

int spdy_surface_model_create(spdy_plan *p, const spdy_surface_clim *host, double delt, int flags, spdy_surface_model **out)
{
    return spdy_ens_surface_model_create(p, 1, host, delt, flags, out);
}

int spdy_ens_surface_model_create(spdy_plan *p, int nmem, const spdy_surface_clim *host, double delt, int flags, spdy_surface_model **out)
{
    NEED_PLAN(p);
    if (nmem < 1 || nmem > 65535) return fail(SPDY_ERR_ARG, "surface_model_create: nmem=%d is not in 1 .. 65535", nmem);
    if (!host || !out) return fail(SPDY_ERR_ARG, "null climatology or result pointer");
    if (flags & ~SPDY_SURFACE_DEFAULT) return fail(SPDY_ERR_ARG, "surface_model_create: unknown flag in %d", flags);
    const bool ssta = flags & SPDY_SURFACE_SST_ANOMALY;
    if (!host->fmask || !host->alb0 || !host->stl12 || !host->snowd12 || !host->soilw12 || !host->sst12 || !host->sice12 ||
        (ssta && !host->sstan3))
        return fail(SPDY_ERR_ARG, "surface_model_create: null field");
    NOT_CAPTURING(p, "spdy_surface_model_create (host table build + upload)");
    spdy_surface_model *m = new spdy_surface_model;
    adopt(p, m);
    m->flags = flags; m->nmem = nmem; m->ncol = grid_elems(p);
    auto cleanup = [&](int rc) { spdy_surface_model_destroy(m); *out = nullptr; return rc; };
    const std::string err = m->tab.build(p->tab, host->fmask, host->alb0, delt);
    if (!err.empty()) return cleanup(fail(SPDY_ERR_ARG, "surface_model_create: %s", err.c_str()));
    *out = m;
    if (p->device < 0) return SPDY_OK;
    if (hipSetDevice(p->device) != hipSuccess) return cleanup(fail(SPDY_ERR_HIP, "hipSetDevice failed"));
    const size_t n = m->ncol, total = (size_t)spdy::surf_total(nmem) * n, bytes = total * sizeof(double);
    if (int rc = dev_alloc(p, bytes, &m->d_f)) return cleanup(rc);
    if (int rc = dev_alloc(p, sizeof(spdy::SurfDate), &m->d_date)) return cleanup(rc);
    // one staging array: the constants, zeros for the model's own fields, the climatologies
    std::vector<double> h(total, 0.0);
    auto put = [&](int at, const double *src, int nf, int e = 0) {
        std::memcpy(h.data() + (size_t)spdy::surf_slot(at, nmem, e) * n, src, sizeof(double) * n * nf);
    };
    const spdy::SurfaceTables &t = m->tab;
    for (int e = 0; e < nmem; ++e) put(spdy::SM_FMASK_L, t.fmask_l.data(), 1, e);
    put(spdy::SM_FMASK_S, t.fmask_s.data(), 1); put(spdy::SM_ALB0, host->alb0, 1);
    put(spdy::SM_RHCAPL, t.rhcapl.data(), 1); put(spdy::SM_CDLAND, t.cdland.data(), 1); put(spdy::SM_RHCAPS, t.rhcaps.data(), 1);
    put(spdy::SM_RHCAPI, t.rhcapi.data(), 1); put(spdy::SM_CDSEA, t.cdsea.data(), 1); put(spdy::SM_CDICE, t.cdice.data(), 1);
    put(spdy::SM_STL12, host->stl12, 12); put(spdy::SM_SNOWD12, host->snowd12, 12); put(spdy::SM_SOILW12, host->soilw12, 12);
    put(spdy::SM_SST12, host->sst12, 12); put(spdy::SM_SICE12, host->sice12, 12);
    if (ssta) put(spdy::SM_SSTAN3, host->sstan3, 3);
    const int rc = upload_sync(p, m->d_f, h.data(), bytes);
    return rc ? cleanup(rc) : SPDY_OK;
}

int spdy_surface_model_destroy(spdy_surface_model *m)
{
    if (!m) return SPDY_OK;
    retire(m, {m->d_f, m->d_date});
    delete m;
    return SPDY_OK;
}

int spdy_surface_model_table(const spdy_surface_model *m, const char *name, double *buf, int cap)
{
    NEED_LIVE(m, "surface model");
    if (!name) return fail(SPDY_ERR_ARG, "null table name");
    const std::vector<double> *v = m->tab.lookup(name);
    if (!v) return fail(SPDY_ERR_ARG, "unknown surface-model table '%s'", name);
    const int n = static_cast<int>(v->size());
    if (buf && cap > 0) std::memcpy(buf, v->data(), sizeof(double) * (size_t)(n < cap ? n : cap));
    return n;
}

int spdy_surface_model_set_date(spdy_surface_model *m, int imont1, double tmonth, double tyear)
{
    NEED_LIVE(m, "surface model");
    spdy_plan *p = m->plan;
    NOT_CAPTURING(p, "spdy_surface_model_set_date (host weights + upload)");
    spdy::SurfaceDateWeights w;
    const std::string err = spdy::surface_date_weights(imont1, tmonth, &w);
    if (!err.empty()) return fail(SPDY_ERR_ARG, "surface_model_set_date: %s", err.c_str());
    NEED_DEVICE(p);
    // the radiation date first: where it is refused (tyear not a number) the model keeps its interpolation date too
    RC(spdy_radiation_set_date(p, tyear));
    spdy::SurfDate d{};
    for (int k = 0; k < 5; ++k) { d.w5[k] = w.w5[k]; d.m5[k] = w.m5[k]; }
    d.wmon = w.wmon; d.m2[0] = w.m2[0]; d.m2[1] = w.m2[1]; d.s2 = w.s2;
    RC(upload_sync(p, m->d_date, &d, sizeof(d)));
    m->date_ready = true;
    return SPDY_OK;
}

int spdy_surface_model_set_sst_anomaly(spdy_surface_model *m, const double *sstan3)
{
    NEED_LIVE(m, "surface model");
    if (!sstan3) return fail(SPDY_ERR_ARG, "null sstan3");
    spdy_plan *p = m->plan;
    NOT_CAPTURING(p, "spdy_surface_model_set_sst_anomaly (upload)");
    NEED_DEVICE(p);
    return upload_sync(p, field(m, spdy::SM_SSTAN3), sstan3, 3 * m->ncol * sizeof(double));
}

int spdy_surface_model_couple_dev(spdy_surface_model *m, int day, const double *hfluxn, const double *shf, const double *evap,
                                  const double *ssrd)
{
    NEED_LIVE(m, "surface model");
    spdy_plan *p = m->plan;
    if (day < 0) return fail(SPDY_ERR_ARG, "surface_model_couple: day %d", day);
    if (day > 0 && !(hfluxn && shf && evap && ssrd)) return fail(SPDY_ERR_ARG, "null device pointer");
    NEED_DEVICE(p);
    if (!m->date_ready) return fail(SPDY_ERR_STATE, "the surface model needs a date (spdy_surface_model_set_date)");
    if (day > 0 && !m->started) return fail(SPDY_ERR_STATE, "the surface model needs couple(day = 0) first");
    // the initialisation marks the model as started: it must have run, not only been recorded
    if (day == 0) NOT_CAPTURING(p, "spdy_surface_model_couple_dev(day = 0)");
    spdy::SurfCols a{};
    a.ncol = (int)m->ncol; a.day = day; a.flags = m->flags; a.f = m->d_f; a.date = m->d_date; a.nmem = m->nmem;
    a.hfluxn = hfluxn; a.shf = shf; a.evap = evap; a.ssrd = ssrd;
    KERNEL(spdy::launch_surface_couple(a, p->stream));
    if (day == 0) m->started = true;
    return SPDY_OK;
}

int spdy_surface_model_forcing_dev(spdy_surface_model *m, double *qcorh)
{
    NEED_LIVE(m, "surface model");
    spdy_plan *p = m->plan;
    if (!qcorh) return fail(SPDY_ERR_ARG, "null device pointer");
    if (m->nmem > p->max_batch) return fail(SPDY_ERR_ARG, "surface_model_forcing: nmem=%d exceeds the plan's max_batch=%d", m->nmem, p->max_batch);
    NEED_DEVICE(p);
    if (!m->date_ready) return fail(SPDY_ERR_STATE, "the surface model needs a date (spdy_surface_model_set_date)");
    if (!m->started) return fail(SPDY_ERR_STATE, "the surface model needs couple(day = 0) first");
    if (!p->tab.orog_ready) return fail(SPDY_ERR_STATE, "the forcing needs the orography (spdy_surface_set_orography)");
    spdy::SurfForcingCols a{};
    a.ncol = (int)m->ncol; a.f = m->d_f; a.phis0 = p->d_orog; a.nmem = m->nmem;
    // forcing.f90:112 gamlat = gamma/(1000. * grav), :86 pexp = 1./(rgas * gamlat)
    a.gamlat = static_cast<double>(6.0f) / (static_cast<double>(1000.0f) * p->tab.grav);
    a.pexp = 1. / (p->tab.rgas * a.gamlat);
    KERNEL(spdy::launch_surface_forcing(a, p->stream));
    // corh of all members is one stack of nmem grids: ONE transform call into the caller's (mx, nx, nmem)
    return spdy_grid_to_spec_dev(p, m->nmem, field(m, spdy::SM_CORH), qcorh);
}

int spdy_surface_model_boundary(spdy_surface_model *m, spdy_sfc_boundary *bnd, const double **albsfc)
{
    NEED_LIVE(m, "surface model");
    if (!bnd || !albsfc) return fail(SPDY_ERR_ARG, "null result pointer");
    NEED_DEVICE(m->plan);
    bnd->fmask = field(m, spdy::SM_FMASK_L); bnd->sst = field(m, spdy::SM_SST_AM); bnd->stl = field(m, spdy::SM_STL_AM);
    bnd->soilw = field(m, spdy::SM_SOILW_AM); bnd->snowc = field(m, spdy::SM_SNOWC); bnd->alb_l = field(m, spdy::SM_ALB_L);
    bnd->alb_s = field(m, spdy::SM_ALB_S);
    *albsfc = field(m, spdy::SM_ALBSFC);
    return SPDY_OK;
}

int spdy_surface_model_field(spdy_surface_model *m, const char *name, double **d_ptr)
{
    NEED_LIVE(m, "surface model");
    if (!name || !d_ptr) return fail(SPDY_ERR_ARG, "null name or result pointer");
    const int i = field_index(name);
    if (i < 0) return fail(SPDY_ERR_ARG, "unknown surface-model field '%s'", name);
    NEED_DEVICE(m->plan);
    *d_ptr = field(m, i);
    return SPDY_OK;
}

int spdy_surface_model_members(const spdy_surface_model *m, const char *name)
{
    NEED_LIVE(m, "surface model");
    if (!name) return m->nmem;
    const int i = field_index(name);
    if (i < 0) return fail(SPDY_ERR_ARG, "unknown surface-model field '%s'", name);
    return spdy::surf_per_member(i) ? m->nmem : 1;
}

}  // extern "C"

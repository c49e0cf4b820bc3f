! bind(C) shim of tests/golden/make_golden_surface.py (test infrastructure only): drives the reference's own
! set_orog_land_sfc_drag, get_surface_fluxes and the boundary-layer block of get_physical_tendencies (physics.f90, cut out by the
! generator into module physics_sfc_ref) on one (ix, il, kx) state.  moist_shim.f90 initialises the geometry and runs the moist
! block, rad_shim.f90 the radiation halves.
subroutine sfc_coa(o_coa) bind(C, name="sfc_coa")
    use iso_c_binding
    use params, only: il
    use geometry, only: coa
    real(c_double), intent(out) :: o_coa(il)
    o_coa = coa
end subroutine

subroutine sfc_tables(o_scal, o_rsig, o_rsig1, o_drh0, o_fvdiq2) bind(C, name="sfc_tables")
    use iso_c_binding
    use params, only: kx
    use physics_sfc_ref, only: vdiff_level_tables
    real(c_double), intent(out) :: o_scal(6), o_rsig(kx), o_rsig1(kx), o_drh0(kx), o_fvdiq2(kx)
    call vdiff_level_tables(o_scal, o_rsig, o_rsig1, o_drh0, o_fvdiq2)
end subroutine

subroutine sfc_orog(phis0, o_forog) bind(C, name="sfc_orog")
    use iso_c_binding
    use params, only: ix, il
    use surface_fluxes, only: set_orog_land_sfc_drag, forog
    real(c_double), intent(in) :: phis0(ix,il)
    real(c_double), intent(out) :: o_forog(ix,il)
    call set_orog_land_sfc_drag(phis0)
    o_forog = forog
end subroutine

subroutine sfc_run(ug, vg, tg, qg, rh, phig, pslg, phis0, fmask, sst, stl, soilw, snowc_in, alb_l_in, alb_s_in, ssrd, slrd, &
        & ustr, vstr, shf, evap, slru, hfluxn, ts, tskin, u0, v0, t0) bind(C, name="sfc_run")
    use iso_c_binding
    use params, only: ix, il, kx
    use mod_radcon, only: alb_l, alb_s, snowc
    use land_model, only: stl_am, soilw_am
    use physics_sfc_ref, only: surface_block
    real(c_double), intent(in) :: ug(ix,il,kx), vg(ix,il,kx), tg(ix,il,kx), qg(ix,il,kx), rh(ix,il,kx), phig(ix,il,kx)
    real(c_double), intent(in) :: pslg(ix,il), phis0(ix,il), fmask(ix,il), sst(ix,il), stl(ix,il), soilw(ix,il)
    real(c_double), intent(in) :: snowc_in(ix,il), alb_l_in(ix,il), alb_s_in(ix,il), ssrd(ix,il), slrd(ix,il)
    real(c_double), intent(out) :: ustr(ix,il,3), vstr(ix,il,3), shf(ix,il,3), evap(ix,il,3), slru(ix,il,3), hfluxn(ix,il,2)
    real(c_double), intent(out) :: ts(ix,il), tskin(ix,il), u0(ix,il), v0(ix,il), t0(ix,il)
    alb_l = alb_l_in
    alb_s = alb_s_in
    snowc = snowc_in
    stl_am = stl
    soilw_am = soilw
    call surface_block(ug, vg, tg, qg, rh, phig, pslg, phis0, fmask, sst, ssrd, slrd, ustr, vstr, shf, evap, slru, hfluxn, ts, &
        & tskin, u0, v0, t0)
end subroutine

subroutine pbl_run(qg, phig, pslg, se, rh, qsat, icnv, ustr, vstr, shf, evap, utend, vtend, ttend, qtend, ut_pbl, vt_pbl, &
        & tt_pbl, qt_pbl) bind(C, name="pbl_run")
    use iso_c_binding
    use params, only: ix, il, kx
    use physics_sfc_ref, only: pbl_block
    real(c_double), intent(in) :: qg(ix,il,kx), phig(ix,il,kx), pslg(ix,il), se(ix,il,kx), rh(ix,il,kx), qsat(ix,il,kx)
    integer(c_int), intent(in) :: icnv(ix,il)
    real(c_double), intent(in) :: ustr(ix,il,3), vstr(ix,il,3), shf(ix,il,3), evap(ix,il,3)
    real(c_double), intent(inout) :: utend(ix,il,kx), vtend(ix,il,kx), ttend(ix,il,kx), qtend(ix,il,kx)
    real(c_double), intent(out) :: ut_pbl(ix,il,kx), vt_pbl(ix,il,kx), tt_pbl(ix,il,kx), qt_pbl(ix,il,kx)
    call pbl_block(qg, phig, pslg, se, rh, qsat, icnv, ustr, vstr, shf, evap, utend, vtend, ttend, qtend, ut_pbl, vt_pbl, &
        & tt_pbl, qt_pbl)
end subroutine

! bind(C) shim of tests/golden/make_golden_radiation.py (test infrastructure only): drives the reference's own radset,
! get_zonal_average_fields and the radiation blocks of get_physical_tendencies (physics.f90, cut out by the generator into
! module physics_rad_ref) on one (ix, il, kx) state.  moist_shim.f90 initialises the geometry and runs the moist block.
subroutine rad_tables(o_fband) bind(C, name="rad_tables")
    use iso_c_binding
    use mod_radcon, only: fband
    use longwave_radiation, only: radset
    real(c_double), intent(out) :: o_fband(100:400,4)
    call radset
    o_fband = fband
end subroutine

subroutine rad_date(tyear, o_fsol, o_ozone, o_ozupp, o_zenit, o_stratz) bind(C, name="rad_date")
    use iso_c_binding
    use params, only: ix, il
    use shortwave_radiation, only: get_zonal_average_fields, fsol, ozone, ozupp, zenit, stratz
    real(c_double), value :: tyear
    real(c_double), intent(out) :: o_fsol(ix,il), o_ozone(ix,il), o_ozupp(ix,il), o_zenit(ix,il), o_stratz(ix,il)
    call get_zonal_average_fields(tyear)
    o_fsol = fsol
    o_ozone = ozone
    o_ozupp = ozupp
    o_zenit = zenit
    o_stratz = stratz
end subroutine

subroutine rad_down(compute_sw, tg, qg, phig, pslg, se, rh, precnv, precls, iptop, fmask, albsfc_in, icltop, cloudc, clstr, &
        & ssrd, ssr, tsr, tt_rsw, slrd, tt_rlw) bind(C, name="rad_down")
    use iso_c_binding
    use params, only: ix, il, kx
    use mod_radcon, only: albsfc
    use shortwave_radiation, only: compute_shortwave
    use physics_rad_ref, only: radiation_down
    integer(c_int), value :: compute_sw
    real(c_double), intent(in) :: tg(ix,il,kx), qg(ix,il,kx), phig(ix,il,kx), pslg(ix,il), se(ix,il,kx), rh(ix,il,kx)
    real(c_double), intent(in) :: precnv(ix,il), precls(ix,il), fmask(ix,il), albsfc_in(ix,il)
    integer(c_int), intent(in) :: iptop(ix,il)
    integer(c_int), intent(inout) :: icltop(ix,il,2)
    real(c_double), intent(inout) :: cloudc(ix,il), clstr(ix,il), ssrd(ix,il), ssr(ix,il), tsr(ix,il), tt_rsw(ix,il,kx)
    real(c_double), intent(inout) :: slrd(ix,il), tt_rlw(ix,il,kx)
    compute_shortwave = compute_sw /= 0
    albsfc = albsfc_in
    call radiation_down(tg, qg, phig, pslg, se, rh, precnv, precls, iptop, fmask, icltop, cloudc, clstr, ssrd, ssr, tsr, &
        & tt_rsw, slrd, tt_rlw)
end subroutine

subroutine rad_up(tg, pslg, ts, slrd, slru, slr, olr, tt_rsw, tt_rlw, ttend) bind(C, name="rad_up")
    use iso_c_binding
    use params, only: ix, il, kx
    use physics_rad_ref, only: radiation_up
    real(c_double), intent(in) :: tg(ix,il,kx), pslg(ix,il), ts(ix,il), slrd(ix,il), slru(ix,il,3), tt_rsw(ix,il,kx)
    real(c_double), intent(inout) :: slr(ix,il), olr(ix,il), tt_rlw(ix,il,kx), ttend(ix,il,kx)
    call radiation_up(tg, pslg, ts, slrd, slru, slr, olr, tt_rsw, tt_rlw, ttend)
end subroutine

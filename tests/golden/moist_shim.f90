! bind(C) shim of tests/golden/make_golden_moist.py (test infrastructure only): drives the reference's own initialize_physics
! and precipitation block (physics.f90, cut out by the generator into module physics_moist_ref) on one (ix, il, kx) state.
subroutine moist_init(have_levels, i_hsg, i_dhs, i_fsg) bind(C, name="moist_init")
    use iso_c_binding
    use params, only: kx
    use geometry, only: initialize_geometry, hsg, dhs, fsg
    use physics_moist_ref, only: initialize_physics
    integer(c_int), value :: have_levels
    real(c_double), intent(in) :: i_hsg(kx+1), i_dhs(kx), i_fsg(kx)
    call initialize_geometry
    if (have_levels /= 0) then      ! a level count the reference has no set for (geometry.f90:42-48)
        hsg = i_hsg
        dhs = i_dhs
        fsg = i_fsg
    end if
    call initialize_physics
end subroutine

subroutine moist_tables(o_sigl, o_sigh, o_grdsig, o_grdscp, o_wvi, o_entr) bind(C, name="moist_tables")
    use iso_c_binding
    use params, only: kx
    use physical_constants, only: sigl, sigh, grdsig, grdscp, wvi
    use physics_moist_ref, only: entrainment
    real(c_double), intent(out) :: o_sigl(kx), o_sigh(0:kx), o_grdsig(kx), o_grdscp(kx), o_wvi(kx,2), o_entr(2:kx-1)
    o_sigl = sigl
    o_sigh = sigh
    o_grdsig = grdsig
    o_grdscp = grdscp
    o_wvi = wvi
    call entrainment(o_entr)
end subroutine

subroutine moist_run(tg, qg, phig, pslg, ttend, qtend, precnv, precls, cbmf, iptop, icnv, qsat, rh, se) bind(C, name="moist_run")
    use iso_c_binding
    use params, only: ix, il, kx
    use physics_moist_ref, only: precipitation_block
    real(c_double), intent(inout) :: tg(ix,il,kx), qg(ix,il,kx), phig(ix,il,kx), pslg(ix,il), ttend(ix,il,kx), qtend(ix,il,kx)
    real(c_double), intent(out) :: precnv(ix,il), precls(ix,il), cbmf(ix,il), qsat(ix,il,kx), rh(ix,il,kx), se(ix,il,kx)
    integer(c_int), intent(out) :: iptop(ix,il), icnv(ix,il)
    call precipitation_block(tg, qg, phig, pslg, ttend, qtend, precnv, precls, cbmf, iptop, icnv, qsat, rh, se)
end subroutine

! bind(C) entry points of tests/golden/make_golden_surfmodel.py into the reference's coupler, land_model, sea_model, date and
! forcing modules, compiled where they lie next to the generator-written stand-in `module input_output` (whose
! load_boundary_file returns the fields sm_inputs puts into its banks).  This file is ours; nothing of the reference is in it
! but the order of its own calls: initialize (initialization.f90:24-60, the parts these modules need) and the main loop's
! body (speedy.f90:29-53) with the caller's flux fields in place of the atmosphere's step.
subroutine sm_inputs(fm, al, ph, b12, sb, nbank) bind(C, name="sm_inputs")
    use iso_c_binding
    use params
    use boundaries, only: fmask, alb0, phis0
    use input_output, only: bank12, ssta_bank, ssta_first
    integer(c_int), value :: nbank
    real(c_double), intent(in) :: fm(ix,il), al(ix,il), ph(ix,il), b12(ix,il,12,5), sb(ix,il,nbank)
    fmask = fm
    alb0 = al
    phis0 = ph
    bank12 = b12
    ssta_bank(:,:,1:nbank) = sb
end subroutine

subroutine sm_init(y, m, d, first) bind(C, name="sm_init")
    use iso_c_binding
    use params
    use date
    use input_output, only: ssta_first
    use geometry, only: initialize_geometry
    use spectral, only: initialize_spectral
    use coupler, only: initialize_coupler
    use forcing, only: set_forcing
    integer(c_int), value :: y, m, d, first
    ssta_first = first                       ! month of the anomaly file that bank slot 1 holds
    call initialize_geometry
    call initialize_spectral
    call initialize_date                     ! the calendar; the dates themselves are set here
    start_datetime%year = y
    start_datetime%month = m
    start_datetime%day = d
    start_datetime%hour = 0
    start_datetime%minute = 0
    model_datetime = start_datetime
    model_datetime%minute = -int(24*60/nsteps)
    call newdate                             ! imont1, tmonth, tyear of the start date, by the reference's own lines
    isst0 = (start_datetime%year - issty0)*12 + start_datetime%month
    call initialize_coupler
    call set_forcing(0)
end subroutine

subroutine sm_step(model_step, hf, sh, ev, ss) bind(C, name="sm_step")
    use iso_c_binding
    use params
    use date, only: newdate
    use auxiliaries, only: hfluxn, shf, evap, ssrd
    use coupler, only: couple_sea_land
    use forcing, only: set_forcing
    integer(c_int), intent(inout) :: model_step
    real(c_double), intent(in) :: hf(ix,il,2), sh(ix,il,3), ev(ix,il,3), ss(ix,il)
    if (mod(model_step-1, nsteps) == 0) call set_forcing(1)
    hfluxn(:,:,1:2) = hf
    shf = sh
    evap = ev
    ssrd = ss
    model_step = model_step + 1
    call newdate
    call couple_sea_land(1+model_step/nsteps)
end subroutine

subroutine sm_get(o, t, r, q, clim, ymdt) bind(C, name="sm_get")
    use iso_c_binding
    use params
    use date
    use land_model
    use sea_model
    use mod_radcon, only: snowc, alb_l, alb_s, albsfc
    use horizontal_diffusion, only: qcorh
    real(c_double), intent(out) :: o(ix,il,19), t(ix,il,8), r(ix,il,4), clim(ix,il,12,5), ymdt(8)
    complex(c_double_complex), intent(out) :: q(mx,nx)
    o(:,:,1) = stlcl_ob; o(:,:,2) = snowdcl_ob; o(:,:,3) = soilwcl_ob; o(:,:,4) = stl_lm; o(:,:,5) = stl_am
    o(:,:,6) = snowd_am; o(:,:,7) = soilw_am; o(:,:,8) = sstcl_ob; o(:,:,9) = sicecl_ob; o(:,:,10) = ticecl_ob
    o(:,:,11) = sstan_ob; o(:,:,12) = sst_om; o(:,:,13) = tice_om; o(:,:,14) = sice_om; o(:,:,15) = sst_am
    o(:,:,16) = sstan_am; o(:,:,17) = sice_am; o(:,:,18) = tice_am; o(:,:,19) = ssti_om
    t(:,:,1) = fmask_l; t(:,:,2) = fmask_s; t(:,:,3) = rhcapl; t(:,:,4) = cdland; t(:,:,5) = rhcaps; t(:,:,6) = rhcapi
    t(:,:,7) = cdsea; t(:,:,8) = cdice
    r(:,:,1) = snowc; r(:,:,2) = alb_l; r(:,:,3) = alb_s; r(:,:,4) = albsfc
    q = qcorh
    clim(:,:,:,1) = stl12; clim(:,:,:,2) = snowd12; clim(:,:,:,3) = soilw12; clim(:,:,:,4) = sst12; clim(:,:,:,5) = sice12
    ymdt = (/ real(model_datetime%year, c_double), real(model_datetime%month, c_double), real(model_datetime%day, c_double), &
        & real(model_datetime%hour, c_double), real(model_datetime%minute, c_double), real(imont1, c_double), tmonth, tyear /)
end subroutine

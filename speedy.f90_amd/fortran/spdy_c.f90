!> ISO_C_BINDING interfaces to the C ABI of include/spdy.h (libspdy.so).
!  One-to-one with the header; complex(c_double_complex) arrays are passed where the C side
!  takes `double*` of interleaved (re,im) pairs -- the storage is identical.
module spdy_c
    use iso_c_binding
    implicit none
    public

    !> spdy_spec_seg (include/spdy.h): one source array of plain spectra of spdy_inverse_batch_segs_dev
    type, bind(C) :: spdy_spec_seg
        integer(c_int) :: nb
        type(c_ptr) :: d_spec
    end type

    !> spdy_hdiff_op, spdy_step_op (include/spdy.h): one array of spdy_hdiff_multi_dev / spdy_step_fields_dev
    type, bind(C) :: spdy_hdiff_op
        integer(c_int) :: nlev
        type(c_ptr) :: field, fdt_in, d_dmp, d_dmp1, fdt_out
    end type
    type, bind(C) :: spdy_step_op
        integer(c_int) :: nlev
        type(c_ptr) :: field, fdt
    end type

    !> spdy_moist_out (include/spdy.h): optional outputs of the moist physics (c_null_ptr = not written)
    type, bind(C) :: spdy_moist_out
        type(c_ptr) :: precnv = c_null_ptr, precls = c_null_ptr, cbmf = c_null_ptr
        type(c_ptr) :: iptop = c_null_ptr, icnv = c_null_ptr
        type(c_ptr) :: qsat = c_null_ptr, rh = c_null_ptr, se = c_null_ptr
    end type

    !> spdy_rad_surface (include/spdy.h): per-column boundary fields of the radiation (land fraction, surface albedo)
    type, bind(C) :: spdy_rad_surface
        type(c_ptr) :: fmask = c_null_ptr, albsfc = c_null_ptr
    end type

    !> spdy_rad_out (include/spdy.h): optional outputs of the radiation (c_null_ptr = not written)
    type, bind(C) :: spdy_rad_out
        type(c_ptr) :: cloudc = c_null_ptr, clstr = c_null_ptr, icltop = c_null_ptr
        type(c_ptr) :: ssrd = c_null_ptr, ssr = c_null_ptr, tsr = c_null_ptr
        type(c_ptr) :: slrd = c_null_ptr, slr = c_null_ptr, olr = c_null_ptr
        type(c_ptr) :: tt_rsw = c_null_ptr, tt_rlw = c_null_ptr
    end type

    !> spdy_surface_clim (include/spdy.h): the host arrays a surface model is made from (c_loc of the caller's fields)
    type, bind(C) :: spdy_surface_clim
        type(c_ptr) :: fmask = c_null_ptr, alb0 = c_null_ptr, stl12 = c_null_ptr, snowd12 = c_null_ptr, soilw12 = c_null_ptr
        type(c_ptr) :: sst12 = c_null_ptr, sice12 = c_null_ptr, sstan3 = c_null_ptr
    end type

    !> spdy_sfc_boundary (include/spdy.h): per-column boundary fields of the surface fluxes, all required
    type, bind(C) :: spdy_sfc_boundary
        type(c_ptr) :: fmask = c_null_ptr, sst = c_null_ptr, stl = c_null_ptr, soilw = c_null_ptr
        type(c_ptr) :: snowc = c_null_ptr, alb_l = c_null_ptr, alb_s = c_null_ptr
    end type

    !> spdy_sfc_out (include/spdy.h): optional outputs of the surface fluxes (c_null_ptr = not written)
    type, bind(C) :: spdy_sfc_out
        type(c_ptr) :: ustr = c_null_ptr, vstr = c_null_ptr, shf = c_null_ptr, evap = c_null_ptr, slru = c_null_ptr
        type(c_ptr) :: hfluxn = c_null_ptr
        type(c_ptr) :: tskin = c_null_ptr, u0 = c_null_ptr, v0 = c_null_ptr, t0 = c_null_ptr
    end type

    !> spdy_pbl_out (include/spdy.h): optional outputs of the boundary layer (c_null_ptr = not written)
    type, bind(C) :: spdy_pbl_out
        type(c_ptr) :: ut_pbl = c_null_ptr, vt_pbl = c_null_ptr, tt_pbl = c_null_ptr, qt_pbl = c_null_ptr
    end type

    !> spdy_column_physics_out (include/spdy.h): the optional outputs of every block of the chain, and ts / fsfcu
    type, bind(C) :: spdy_column_physics_out
        type(spdy_moist_out) :: moist
        type(spdy_rad_out) :: rad
        type(spdy_sfc_out) :: sfc
        type(spdy_pbl_out) :: pbl
        type(c_ptr) :: ts = c_null_ptr, fsfcu = c_null_ptr
    end type

    !> spdy_output_fields (include/spdy.h): one group of float fields of spdy_ens_output_batch_dev, all six required
    type, bind(C) :: spdy_output_fields
        type(c_ptr) :: u = c_null_ptr, v = c_null_ptr, t = c_null_ptr, q = c_null_ptr, phi = c_null_ptr, ps = c_null_ptr
    end type

    !> spdy_obs (include/spdy.h, "ensemble analysis"): var SPDY_OBS_*, lev 0-based (ignored for PS), degrees, the model's units
    type, bind(C) :: spdy_obs
        integer(c_int) :: var = 0_c_int, lev = 0_c_int
        real(c_double) :: lon = 0.0_c_double, lat = 0.0_c_double, value = 0.0_c_double, error = 1.0_c_double
    end type

    !> spdy_pobs (include/spdy.h, "observations at a pressure"): spdy_obs with p in Pa, read where lev = SPDY_OBS_AT_P
    type, bind(C) :: spdy_pobs
        integer(c_int) :: var = 0_c_int, lev = 0_c_int
        real(c_double) :: p = 0.0_c_double, lon = 0.0_c_double, lat = 0.0_c_double, value = 0.0_c_double, error = 1.0_c_double
    end type

    interface
        function spdy_plan_create(trunc, ix, iy, kx, max_batch, device, plan) bind(C, name="spdy_plan_create") result(rc)
            import :: c_int, c_ptr
            integer(c_int), value :: trunc, ix, iy, kx, max_batch, device
            type(c_ptr), intent(out) :: plan
            integer(c_int) :: rc
        end function
        function spdy_plan_destroy(plan) bind(C, name="spdy_plan_destroy") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int) :: rc
        end function
        function spdy_last_error() bind(C, name="spdy_last_error") result(msg)
            import :: c_ptr
            type(c_ptr) :: msg
        end function
        function spdy_get_table(plan, name, buf, cap) bind(C, name="spdy_get_table") result(rc)
            import :: c_int, c_ptr, c_char, c_double
            type(c_ptr), value :: plan
            character(kind=c_char), intent(in) :: name(*)
            real(c_double), intent(out) :: buf(*)
            integer(c_int), value :: cap
            integer(c_int) :: rc
        end function
        function spdy_spec_to_grid(plan, spec, kcos, grid) bind(C, name="spdy_spec_to_grid") result(rc)
            import :: c_int, c_ptr, c_double, c_double_complex
            type(c_ptr), value :: plan
            complex(c_double_complex), intent(in) :: spec(*)
            integer(c_int), value :: kcos
            real(c_double), intent(out) :: grid(*)
            integer(c_int) :: rc
        end function
        function spdy_grid_to_spec(plan, grid, spec) bind(C, name="spdy_grid_to_spec") result(rc)
            import :: c_int, c_ptr, c_double, c_double_complex
            type(c_ptr), value :: plan
            real(c_double), intent(in) :: grid(*)
            complex(c_double_complex), intent(out) :: spec(*)
            integer(c_int) :: rc
        end function
        function spdy_spec_to_grid_batch(plan, nb, spec, kcos, grid) bind(C, name="spdy_spec_to_grid_batch") result(rc)
            import :: c_int, c_ptr, c_double, c_double_complex
            type(c_ptr), value :: plan
            integer(c_int), value :: nb
            complex(c_double_complex), intent(in) :: spec(*)
            integer(c_int), intent(in) :: kcos(*)
            real(c_double), intent(out) :: grid(*)
            integer(c_int) :: rc
        end function
        function spdy_grid_to_spec_batch(plan, nb, grid, spec) bind(C, name="spdy_grid_to_spec_batch") result(rc)
            import :: c_int, c_ptr, c_double, c_double_complex
            type(c_ptr), value :: plan
            integer(c_int), value :: nb
            real(c_double), intent(in) :: grid(*)
            complex(c_double_complex), intent(out) :: spec(*)
            integer(c_int) :: rc
        end function
        function spdy_laplacian(plan, nb, a, o) bind(C, name="spdy_laplacian") result(rc)
            import :: c_int, c_ptr, c_double_complex
            type(c_ptr), value :: plan
            integer(c_int), value :: nb
            complex(c_double_complex), intent(in) :: a(*)
            complex(c_double_complex), intent(out) :: o(*)
            integer(c_int) :: rc
        end function
        function spdy_inverse_laplacian(plan, nb, a, o) bind(C, name="spdy_inverse_laplacian") result(rc)
            import :: c_int, c_ptr, c_double_complex
            type(c_ptr), value :: plan
            integer(c_int), value :: nb
            complex(c_double_complex), intent(in) :: a(*)
            complex(c_double_complex), intent(out) :: o(*)
            integer(c_int) :: rc
        end function
        function spdy_trunct(plan, nb, a) bind(C, name="spdy_trunct") result(rc)
            import :: c_int, c_ptr, c_double_complex
            type(c_ptr), value :: plan
            integer(c_int), value :: nb
            complex(c_double_complex), intent(inout) :: a(*)
            integer(c_int) :: rc
        end function
        function spdy_grad(plan, nb, psi, psdx, psdy) bind(C, name="spdy_grad") result(rc)
            import :: c_int, c_ptr, c_double_complex
            type(c_ptr), value :: plan
            integer(c_int), value :: nb
            complex(c_double_complex), intent(in) :: psi(*)
            complex(c_double_complex), intent(inout) :: psdx(*), psdy(*)
            integer(c_int) :: rc
        end function
        function spdy_vds(plan, nb, ucosm, vcosm, vorm, divm) bind(C, name="spdy_vds") result(rc)
            import :: c_int, c_ptr, c_double_complex
            type(c_ptr), value :: plan
            integer(c_int), value :: nb
            complex(c_double_complex), intent(in) :: ucosm(*), vcosm(*)
            complex(c_double_complex), intent(inout) :: vorm(*), divm(*)
            integer(c_int) :: rc
        end function
        function spdy_uvspec(plan, nb, vorm, divm, ucosm, vcosm) bind(C, name="spdy_uvspec") result(rc)
            import :: c_int, c_ptr, c_double_complex
            type(c_ptr), value :: plan
            integer(c_int), value :: nb
            complex(c_double_complex), intent(in) :: vorm(*), divm(*)
            complex(c_double_complex), intent(inout) :: ucosm(*), vcosm(*)
            integer(c_int) :: rc
        end function
        function spdy_vdspec(plan, nb, ug, vg, vorm, divm, kcos) bind(C, name="spdy_vdspec") result(rc)
            import :: c_int, c_ptr, c_double, c_double_complex
            type(c_ptr), value :: plan
            integer(c_int), value :: nb, kcos
            real(c_double), intent(in) :: ug(*), vg(*)
            complex(c_double_complex), intent(out) :: vorm(*), divm(*)
            integer(c_int) :: rc
        end function
        function spdy_uvspec_to_grid(plan, nb, vorm, divm, ug, vg, kcos) bind(C, name="spdy_uvspec_to_grid") result(rc)
            import :: c_ptr, c_int, c_double, c_double_complex
            type(c_ptr), value :: plan
            integer(c_int), value :: nb, kcos
            complex(c_double_complex), intent(in) :: vorm(*), divm(*)
            real(c_double), intent(out) :: ug(*), vg(*)
            integer(c_int) :: rc
        end function
        function spdy_grad_to_grid(plan, nb, psi, gx, gy, kcos) bind(C, name="spdy_grad_to_grid") result(rc)
            import :: c_ptr, c_int, c_double, c_double_complex
            type(c_ptr), value :: plan
            integer(c_int), value :: nb, kcos
            complex(c_double_complex), intent(in) :: psi(*)
            real(c_double), intent(out) :: gx(*), gy(*)
            integer(c_int) :: rc
        end function
        function spdy_hdiff(plan, nlev, field, fdt_in, dmp, dmp1, fdt_out) bind(C, name="spdy_hdiff") result(rc)
            import :: c_int, c_ptr, c_double, c_double_complex
            type(c_ptr), value :: plan
            integer(c_int), value :: nlev
            complex(c_double_complex), intent(in) :: field(*), fdt_in(*)
            real(c_double), intent(in) :: dmp(*), dmp1(*)
            complex(c_double_complex), intent(out) :: fdt_out(*)
            integer(c_int) :: rc
        end function
        function spdy_implicit_init(plan, dt) bind(C, name="spdy_implicit_init") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: plan
            real(c_double), value :: dt
            integer(c_int) :: rc
        end function
        function spdy_implicit_terms(plan, divdt, tdt, psdt) bind(C, name="spdy_implicit_terms") result(rc)
            import :: c_int, c_ptr, c_double_complex
            type(c_ptr), value :: plan
            complex(c_double_complex), intent(inout) :: divdt(*), tdt(*), psdt(*)
            integer(c_int) :: rc
        end function
        function spdy_plan_set_sigma(plan, hsg) bind(C, name="spdy_plan_set_sigma") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: plan
            real(c_double), intent(in) :: hsg(*)
            integer(c_int) :: rc
        end function
        function spdy_geopotential(plan, t, phis, phi) bind(C, name="spdy_geopotential") result(rc)
            import :: c_int, c_ptr, c_double_complex
            type(c_ptr), value :: plan
            complex(c_double_complex), intent(in) :: t(*), phis(*)
            complex(c_double_complex), intent(out) :: phi(*)
            integer(c_int) :: rc
        end function
        function spdy_step_field(plan, nlev, j1, dt, eps, wil, field, fdt) bind(C, name="spdy_step_field") result(rc)
            import :: c_int, c_ptr, c_double, c_double_complex
            type(c_ptr), value :: plan
            integer(c_int), value :: nlev, j1
            real(c_double), value :: dt, eps, wil
            complex(c_double_complex), intent(inout) :: field(*), fdt(*)
            integer(c_int) :: rc
        end function
        ! ---- multi-GPU (one process per GPU): level all-gather over RCCL for the level-sharded implicit solve
        function spdy_comm_unique_id(id) bind(C, name="spdy_comm_unique_id") result(rc)
            import :: c_int, c_char
            character(kind=c_char), intent(out) :: id(128)
            integer(c_int) :: rc
        end function
        function spdy_comm_create(plan, nranks, rank, id, comm) bind(C, name="spdy_comm_create") result(rc)
            import :: c_int, c_ptr, c_char
            type(c_ptr), value :: plan
            integer(c_int), value :: nranks, rank
            character(kind=c_char), intent(in) :: id(128)
            type(c_ptr), intent(out) :: comm
            integer(c_int) :: rc
        end function
        function spdy_comm_destroy(comm) bind(C, name="spdy_comm_destroy") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: comm
            integer(c_int) :: rc
        end function
        function spdy_comm_level_range(comm, nlev, lo, hi) bind(C, name="spdy_comm_level_range") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: comm
            integer(c_int), value :: nlev
            integer(c_int), intent(out) :: lo, hi
            integer(c_int) :: rc
        end function
        ! device pointers (type(c_ptr) values obtained from the host's own HIP allocations)
        function spdy_implicit_terms_sharded_dev(comm, divdt, tdt, psdt) bind(C, name="spdy_implicit_terms_sharded_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: comm, divdt, tdt, psdt
            integer(c_int) :: rc
        end function
        ! ---- device-resident state: memory, the step's entry points, graph capture (time_stepping.f90) ----------
        function spdy_plan_synchronize(plan) bind(C, name="spdy_plan_synchronize") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int) :: rc
        end function
        function spdy_dev_alloc(plan, bytes, d_ptr) bind(C, name="spdy_dev_alloc") result(rc)
            import :: c_int, c_ptr, c_size_t
            type(c_ptr), value :: plan
            integer(c_size_t), value :: bytes
            type(c_ptr), intent(out) :: d_ptr
            integer(c_int) :: rc
        end function
        function spdy_dev_free(plan, d_ptr) bind(C, name="spdy_dev_free") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, d_ptr
            integer(c_int) :: rc
        end function
        ! host side as type(*): any contiguous array (complex or real) goes up or comes down as bytes
        function spdy_dev_upload(plan, d_dst, src, bytes) bind(C, name="spdy_dev_upload") result(rc)
            import :: c_int, c_ptr, c_size_t
            type(c_ptr), value :: plan, d_dst
            type(*), intent(in) :: src(*)
            integer(c_size_t), value :: bytes
            integer(c_int) :: rc
        end function
        function spdy_dev_download(plan, dst, d_src, bytes) bind(C, name="spdy_dev_download") result(rc)
            import :: c_int, c_ptr, c_size_t
            type(c_ptr), value :: plan, d_src
            type(*) :: dst(*)
            integer(c_size_t), value :: bytes
            integer(c_int) :: rc
        end function
        function spdy_graph_begin(plan) bind(C, name="spdy_graph_begin") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int) :: rc
        end function
        function spdy_graph_end(plan, graph) bind(C, name="spdy_graph_end") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            type(c_ptr), intent(out) :: graph
            integer(c_int) :: rc
        end function
        function spdy_graph_launch(graph) bind(C, name="spdy_graph_launch") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: graph
            integer(c_int) :: rc
        end function
        function spdy_comm_set_option(comm, name, value) bind(C, name="spdy_comm_set_option") result(rc)
            import :: c_char, c_int, c_ptr
            type(c_ptr), value :: comm
            character(kind=c_char), intent(in) :: name(*)     ! NUL-terminated
            integer(c_int), value :: value
            integer(c_int) :: rc
        end function
        function spdy_sharded_state_gather_dev(comm, vor, div, t, tr, ps) bind(C, name="spdy_sharded_state_gather_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: comm, vor, div, t, tr, ps
            integer(c_int) :: rc
        end function
        function spdy_sharded_gather_ranges_dev(comm, narr, arrays, nrows) bind(C, name="spdy_sharded_gather_ranges_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: comm
            integer(c_int), value :: narr
            type(c_ptr), intent(in) :: arrays(*)
            integer(c_int), intent(in) :: nrows(*)
            integer(c_int) :: rc
        end function
        function spdy_comm_describe(comm, buf, len) bind(C, name="spdy_comm_describe") result(rc)
            import :: c_char, c_int, c_ptr
            type(c_ptr), value :: comm
            character(kind=c_char), intent(out) :: buf(*)
            integer(c_int), value :: len
            integer(c_int) :: rc
        end function
        function spdy_graph_num_nodes(graph, nodes) bind(C, name="spdy_graph_num_nodes") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: graph
            integer(c_int), intent(out) :: nodes
            integer(c_int) :: rc
        end function
        function spdy_graph_destroy(graph) bind(C, name="spdy_graph_destroy") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: graph
            integer(c_int) :: rc
        end function
        ! every array argument below is a device pointer
        function spdy_inverse_batch_segs_dev(plan, npairs, d_vor, d_div, d_ug, d_vg, kcos_pairs, nseg, segs, d_kcos, kcos_all, &
                & d_grid, ngrad, d_psi, d_gx, d_gy, kcos_grad) bind(C, name="spdy_inverse_batch_segs_dev") result(rc)
            import :: c_int, c_ptr, spdy_spec_seg
            type(c_ptr), value :: plan, d_vor, d_div, d_ug, d_vg, d_kcos, d_grid, d_psi, d_gx, d_gy
            integer(c_int), value :: npairs, kcos_pairs, nseg, kcos_all, ngrad, kcos_grad
            type(spdy_spec_seg), intent(in) :: segs(*)
            integer(c_int) :: rc
        end function
        function spdy_grid_tendencies_dev(plan, ug, vg, tg, vorg, divg, trg, px, py, u_out, v_out, plain_out) &
                & bind(C, name="spdy_grid_tendencies_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, ug, vg, tg, vorg, divg, trg, px, py, u_out, v_out, plain_out
            integer(c_int) :: rc
        end function
        function spdy_direct_batch_spectral_step_dev(plan, d_ug, d_vg, d_grid, kcos, pvor, pdiv, pspec, vor, div, t, tr, ps, &
                & phis, d_tcorh, d_qcorh, sdrag, j1, dt, eps, wil, phi) bind(C, name="spdy_direct_batch_spectral_step_dev") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: plan, d_ug, d_vg, d_grid, pvor, pdiv, pspec, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, phi
            integer(c_int), value :: kcos, j1
            real(c_double), value :: sdrag, dt, eps, wil
            integer(c_int) :: rc
        end function
        ! ---- the rest of include/spdy.h, one interface per entry point (device pointers are type(c_ptr) values) ----
        function spdy_plan_set_stream(plan, hip_stream) bind(C, name="spdy_plan_set_stream") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, hip_stream
            integer(c_int) :: rc
        end function
        function spdy_plan_set_profiling(plan, on) bind(C, name="spdy_plan_set_profiling") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), value :: on
            integer(c_int) :: rc
        end function
        function spdy_plan_set_fused(plan, mode) bind(C, name="spdy_plan_set_fused") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), value :: mode
            integer(c_int) :: rc
        end function
        function spdy_plan_set_option(plan, name, value) bind(C, name="spdy_plan_set_option") result(rc)
            import :: c_char, c_int, c_ptr
            type(c_ptr), value :: plan
            character(kind=c_char), intent(in) :: name(*)     ! NUL-terminated
            integer(c_int), value :: value
            integer(c_int) :: rc
        end function
        function spdy_plan_get_profile(plan, ms, launches) bind(C, name="spdy_plan_get_profile") result(rc)
            import :: c_double, c_int, c_ptr
            type(c_ptr), value :: plan
            real(c_double), intent(out) :: ms(*)
            integer(c_int), intent(out) :: launches(*)
            integer(c_int) :: rc
        end function
        function spdy_wave_placement(plan, simd_of_wave, violations) bind(C, name="spdy_wave_placement") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), intent(out) :: simd_of_wave(8), violations
            integer(c_int) :: rc
        end function
        function spdy_plan_dims(plan, dims) bind(C, name="spdy_plan_dims") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), intent(out) :: dims(*)
            integer(c_int) :: rc
        end function
        function spdy_spec_to_grid_dev(plan, nb, d_spec, d_kcos, kcos_all, d_grid) &
                & bind(C, name="spdy_spec_to_grid_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, d_spec, d_kcos, d_grid
            integer(c_int), value :: nb, kcos_all
            integer(c_int) :: rc
        end function
        function spdy_grid_to_spec_dev(plan, nb, d_grid, d_spec) bind(C, name="spdy_grid_to_spec_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, d_grid, d_spec
            integer(c_int), value :: nb
            integer(c_int) :: rc
        end function
        function spdy_legendre_inv(plan, nb, spec, four) bind(C, name="spdy_legendre_inv") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), value :: nb
            type(*), intent(in) :: spec(*)
            type(*) :: four(*)
            integer(c_int) :: rc
        end function
        function spdy_legendre_dir(plan, nb, four, spec) bind(C, name="spdy_legendre_dir") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), value :: nb
            type(*), intent(in) :: four(*)
            type(*) :: spec(*)
            integer(c_int) :: rc
        end function
        function spdy_fourier_inv(plan, nb, four, kcos, grid) bind(C, name="spdy_fourier_inv") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), value :: nb, kcos
            type(*), intent(in) :: four(*)
            type(*) :: grid(*)
            integer(c_int) :: rc
        end function
        function spdy_fourier_dir(plan, nb, grid, four) bind(C, name="spdy_fourier_dir") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), value :: nb
            type(*), intent(in) :: grid(*)
            type(*) :: four(*)
            integer(c_int) :: rc
        end function
        function spdy_laplacian_dev(plan, nb, in, out) bind(C, name="spdy_laplacian_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, in, out
            integer(c_int), value :: nb
            integer(c_int) :: rc
        end function
        function spdy_inverse_laplacian_dev(plan, nb, in, out) bind(C, name="spdy_inverse_laplacian_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, in, out
            integer(c_int), value :: nb
            integer(c_int) :: rc
        end function
        function spdy_trunct_dev(plan, nb, inout) bind(C, name="spdy_trunct_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, inout
            integer(c_int), value :: nb
            integer(c_int) :: rc
        end function
        function spdy_grad_dev(plan, nb, psi, psdx, psdy) bind(C, name="spdy_grad_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, psi, psdx, psdy
            integer(c_int), value :: nb
            integer(c_int) :: rc
        end function
        function spdy_vds_dev(plan, nb, ucosm, vcosm, vorm, divm) bind(C, name="spdy_vds_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, ucosm, vcosm, vorm, divm
            integer(c_int), value :: nb
            integer(c_int) :: rc
        end function
        function spdy_uvspec_dev(plan, nb, vorm, divm, ucosm, vcosm) bind(C, name="spdy_uvspec_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, vorm, divm, ucosm, vcosm
            integer(c_int), value :: nb
            integer(c_int) :: rc
        end function
        function spdy_vdspec_dev(plan, nb, ug, vg, vorm, divm, kcos) bind(C, name="spdy_vdspec_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, ug, vg, vorm, divm
            integer(c_int), value :: nb, kcos
            integer(c_int) :: rc
        end function
        function spdy_hdiff_dev(plan, nlev, field, fdt_in, d_dmp, d_dmp1, fdt_out) bind(C, name="spdy_hdiff_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, field, fdt_in, d_dmp, d_dmp1, fdt_out
            integer(c_int), value :: nlev
            integer(c_int) :: rc
        end function
        function spdy_hdiff_multi_dev(plan, nops, ops) bind(C, name="spdy_hdiff_multi_dev") result(rc)
            import :: c_int, c_ptr, spdy_hdiff_op
            type(c_ptr), value :: plan
            integer(c_int), value :: nops
            type(spdy_hdiff_op), intent(in) :: ops(*)
            integer(c_int) :: rc
        end function
        function spdy_implicit_terms_dev(plan, divdt, tdt, psdt) bind(C, name="spdy_implicit_terms_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, divdt, tdt, psdt
            integer(c_int) :: rc
        end function
        function spdy_device_table(plan, name, d_ptr) bind(C, name="spdy_device_table") result(rc)
            import :: c_char, c_int, c_ptr
            type(c_ptr), value :: plan
            character(kind=c_char), intent(in) :: name(*)
            type(c_ptr), intent(out) :: d_ptr
            integer(c_int) :: rc
        end function
        function spdy_geopotential_dev(plan, t, phis, phi) bind(C, name="spdy_geopotential_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, t, phis, phi
            integer(c_int) :: rc
        end function
        function spdy_spectral_tendencies_dev(plan, div, t, ps, phis, divdt, tdt, psdt, phi) &
                & bind(C, name="spdy_spectral_tendencies_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, div, t, ps, phis, divdt, tdt, psdt, phi
            integer(c_int) :: rc
        end function
        function spdy_hdiff_step_dev(plan, vor, div, t, tr, d_tcorh, d_qcorh, sdrag, vordt, divdt, tdt, trdt) &
                & bind(C, name="spdy_hdiff_step_dev") result(rc)
            import :: c_double, c_int, c_ptr
            type(c_ptr), value :: plan, vor, div, t, tr, d_tcorh, d_qcorh, vordt, divdt, tdt, trdt
            real(c_double), value :: sdrag
            integer(c_int) :: rc
        end function
        function spdy_step_fields_dev(plan, nops, ops, j1, dt, eps, wil) bind(C, name="spdy_step_fields_dev") result(rc)
            import :: c_double, c_int, c_ptr, spdy_step_op
            type(c_ptr), value :: plan
            integer(c_int), value :: nops, j1
            type(spdy_step_op), intent(in) :: ops(*)
            real(c_double), value :: dt, eps, wil
            integer(c_int) :: rc
        end function
        function spdy_tendency_combine_dev(plan, pdiv, pspec) bind(C, name="spdy_tendency_combine_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, pdiv, pspec
            integer(c_int) :: rc
        end function
        function spdy_spectral_step_dev(plan, pvor, pdiv, pspec, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, sdrag, j1, &
                & dt, eps, wil, phi) &
                & bind(C, name="spdy_spectral_step_dev") result(rc)
            import :: c_double, c_int, c_ptr
            type(c_ptr), value :: plan, pvor, pdiv, pspec, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, phi
            real(c_double), value :: sdrag, dt, eps, wil
            integer(c_int), value :: j1
            integer(c_int) :: rc
        end function
        function spdy_allgather_levels_dev(comm, nlev, narr, d_full) bind(C, name="spdy_allgather_levels_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: comm
            integer(c_int), value :: nlev, narr
            type(c_ptr), intent(in) :: d_full(*)
            integer(c_int) :: rc
        end function
        ! ranks inside one process (one host thread + one plan per GPU) and the complete level-sharded step
        function spdy_comm_group_create(nranks, group) bind(C, name="spdy_comm_group_create") result(rc)
            import :: c_int, c_ptr
            integer(c_int), value :: nranks
            type(c_ptr), intent(out) :: group
            integer(c_int) :: rc
        end function
        function spdy_comm_group_destroy(group) bind(C, name="spdy_comm_group_destroy") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: group
            integer(c_int) :: rc
        end function
        function spdy_comm_create_local(plan, group, rank, comm) bind(C, name="spdy_comm_create_local") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, group
            integer(c_int), value :: rank
            type(c_ptr), intent(out) :: comm
            integer(c_int) :: rc
        end function
        function spdy_sharded_step_workspace(comm) bind(C, name="spdy_sharded_step_workspace") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: comm
            integer(c_int) :: rc
        end function
        function spdy_sharded_step_dev(comm, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, sdrag, j1, j2, dt, eps, wil, phi, tend_out) &
                & bind(C, name="spdy_sharded_step_dev") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: comm, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, phi, tend_out
            real(c_double), value :: sdrag, dt, eps, wil
            integer(c_int), value :: j1, j2
            integer(c_int) :: rc
        end function
        function spdy_sharded_step_grid_dev(comm, vor, div, t, tr, ps, j2) bind(C, name="spdy_sharded_step_grid_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: comm, vor, div, t, tr, ps
            integer(c_int), value :: j2
            integer(c_int) :: rc
        end function
        function spdy_sharded_step_operands(comm, u, v, plain, lo, hi) bind(C, name="spdy_sharded_step_operands") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: comm
            type(c_ptr), intent(out) :: u, v, plain
            integer(c_int), intent(out) :: lo, hi
            integer(c_int) :: rc
        end function
        function spdy_sharded_step_spectral_dev(comm, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, sdrag, j1, dt, eps, wil, phi, &
                & tend_out) bind(C, name="spdy_sharded_step_spectral_dev") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: comm, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, phi, tend_out
            real(c_double), value :: sdrag, dt, eps, wil
            integer(c_int), value :: j1
            integer(c_int) :: rc
        end function
        function spdy_sharded_step_stacks(comm, grid_stack, grid_doubles, spec_stack, spec_doubles) &
                & bind(C, name="spdy_sharded_step_stacks") result(rc)
            import :: c_int, c_ptr, c_size_t
            type(c_ptr), value :: comm
            type(c_ptr), intent(out) :: grid_stack, spec_stack
            integer(c_size_t), intent(out) :: grid_doubles, spec_doubles
            integer(c_int) :: rc
        end function
        function spdy_uvspec_to_grid_dev(plan, nb, d_vor, d_div, d_ug, d_vg, kcos) &
                & bind(C, name="spdy_uvspec_to_grid_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, d_vor, d_div, d_ug, d_vg
            integer(c_int), value :: nb, kcos
            integer(c_int) :: rc
        end function
        function spdy_grad_to_grid_dev(plan, nb, d_psi, d_gx, d_gy, kcos) bind(C, name="spdy_grad_to_grid_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, d_psi, d_gx, d_gy
            integer(c_int), value :: nb, kcos
            integer(c_int) :: rc
        end function
        function spdy_inverse_batch_dev(plan, npairs, d_vor, d_div, d_ug, d_vg, kcos_pairs, nplain, d_spec, d_kcos, &
                & kcos_all, d_grid) &
                & bind(C, name="spdy_inverse_batch_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, d_vor, d_div, d_ug, d_vg, d_spec, d_kcos, d_grid
            integer(c_int), value :: npairs, kcos_pairs, nplain, kcos_all
            integer(c_int) :: rc
        end function
        function spdy_direct_batch_dev(plan, npairs, d_ug, d_vg, d_vorm, d_divm, kcos, nplain, d_grid, d_spec) &
                & bind(C, name="spdy_direct_batch_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, d_ug, d_vg, d_vorm, d_divm, d_grid, d_spec
            integer(c_int), value :: npairs, kcos, nplain
            integer(c_int) :: rc
        end function
        function spdy_inverse_batch_grad_dev(plan, npairs, d_vor, d_div, d_ug, d_vg, kcos_pairs, nplain, d_spec, d_kcos, &
                & kcos_all, d_grid, ngrad, d_psi, d_gx, d_gy, kcos_grad) &
                & bind(C, name="spdy_inverse_batch_grad_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, d_vor, d_div, d_ug, d_vg, d_spec, d_kcos, d_grid, d_psi, d_gx, d_gy
            integer(c_int), value :: npairs, kcos_pairs, nplain, kcos_all, ngrad, kcos_grad
            integer(c_int) :: rc
        end function
        function spdy_moist_columns_dev(plan, nb, tg, qg, phig, pslg, ttend, qtend, out) &
                & bind(C, name="spdy_moist_columns_dev") result(rc)
            import :: c_int, c_ptr, spdy_moist_out
            type(c_ptr), value :: plan, tg, qg, phig, pslg, ttend, qtend
            integer(c_int), value :: nb
            type(spdy_moist_out), intent(in) :: out
            integer(c_int) :: rc
        end function
        function spdy_moist_workspace(plan) bind(C, name="spdy_moist_workspace") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int) :: rc
        end function
        function spdy_moist_physics_dev(plan, t, q, phi, ps, ttend, qtend, out) &
                & bind(C, name="spdy_moist_physics_dev") result(rc)
            import :: c_int, c_ptr, spdy_moist_out
            type(c_ptr), value :: plan, t, q, phi, ps, ttend, qtend
            type(spdy_moist_out), intent(in) :: out
            integer(c_int) :: rc
        end function
        function spdy_radiation_set_date(plan, tyear) bind(C, name="spdy_radiation_set_date") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: plan
            real(c_double), value :: tyear
            integer(c_int) :: rc
        end function
        function spdy_radiation_state_size(plan) bind(C, name="spdy_radiation_state_size") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int) :: rc
        end function
        function spdy_radiation_down_dev(plan, nb, compute_sw, tg, qg, phig, pslg, rh, precnv, precls, iptop, sfc, state, out) &
                & bind(C, name="spdy_radiation_down_dev") result(rc)
            import :: c_int, c_ptr, spdy_rad_surface, spdy_rad_out
            type(c_ptr), value :: plan, tg, qg, phig, pslg, rh, precnv, precls, iptop, state
            integer(c_int), value :: nb, compute_sw
            type(spdy_rad_surface), intent(in) :: sfc
            type(spdy_rad_out), intent(in) :: out
            integer(c_int) :: rc
        end function
        function spdy_radiation_up_dev(plan, nb, tg, pslg, ts, fsfcu, state, ttend, out) &
                & bind(C, name="spdy_radiation_up_dev") result(rc)
            import :: c_int, c_ptr, spdy_rad_out
            type(c_ptr), value :: plan, tg, pslg, ts, fsfcu, state, ttend
            integer(c_int), value :: nb
            type(spdy_rad_out), intent(in) :: out
            integer(c_int) :: rc
        end function
        function spdy_surface_set_orography(plan, phis0) bind(C, name="spdy_surface_set_orography") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, phis0
            integer(c_int) :: rc
        end function
        function spdy_surface_fluxes_dev(plan, nb, ug, vg, tg, qg, phig, pslg, ssrd, slrd, bnd, ts, fsfcu, flux3, out) &
                & bind(C, name="spdy_surface_fluxes_dev") result(rc)
            import :: c_int, c_ptr, spdy_sfc_boundary, spdy_sfc_out
            type(c_ptr), value :: plan, ug, vg, tg, qg, phig, pslg, ssrd, slrd, ts, fsfcu, flux3
            integer(c_int), value :: nb
            type(spdy_sfc_boundary), intent(in) :: bnd
            type(spdy_sfc_out), intent(in) :: out
            integer(c_int) :: rc
        end function
        function spdy_pbl_dev(plan, nb, qg, phig, pslg, se, rh, qsat, icnv, flux3, utend, vtend, ttend, qtend, out) &
                & bind(C, name="spdy_pbl_dev") result(rc)
            import :: c_int, c_ptr, spdy_pbl_out
            type(c_ptr), value :: plan, qg, phig, pslg, se, rh, qsat, icnv, flux3, utend, vtend, ttend, qtend
            integer(c_int), value :: nb
            type(spdy_pbl_out), intent(in) :: out
            integer(c_int) :: rc
        end function
        function spdy_column_physics_workspace(plan) bind(C, name="spdy_column_physics_workspace") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int) :: rc
        end function
        function spdy_column_physics_dev(plan, nb, compute_sw, ug, vg, tg, qg, phig, pslg, bnd, albsfc, rad_state, utend, vtend, &
                & ttend, qtend, out) bind(C, name="spdy_column_physics_dev") result(rc)
            import :: c_int, c_ptr, spdy_sfc_boundary, spdy_column_physics_out
            type(c_ptr), value :: plan, ug, vg, tg, qg, phig, pslg, albsfc, rad_state, utend, vtend, ttend, qtend
            integer(c_int), value :: nb, compute_sw
            type(spdy_sfc_boundary), intent(in) :: bnd
            type(spdy_column_physics_out), intent(in) :: out
            integer(c_int) :: rc
        end function
        function spdy_physics_workspace(plan) bind(C, name="spdy_physics_workspace") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int) :: rc
        end function
        function spdy_physics_dev(plan, compute_sw, vor, div, t, q, phi, ps, bnd, albsfc, rad_state, utend, vtend, ttend, qtend, &
                & out) bind(C, name="spdy_physics_dev") result(rc)
            import :: c_int, c_ptr, spdy_sfc_boundary, spdy_column_physics_out
            type(c_ptr), value :: plan, vor, div, t, q, phi, ps, albsfc, rad_state, utend, vtend, ttend, qtend
            integer(c_int), value :: compute_sw
            type(spdy_sfc_boundary), intent(in) :: bnd
            type(spdy_column_physics_out), intent(in) :: out
            integer(c_int) :: rc
        end function
        ! the ensemble time step (include/spdy.h): nmem members through one step's launches; the drop-in steps one state and does
        ! not call these
        function spdy_ens_grid_tendencies_dev(plan, nmem, ug, vg, tg, vorg, divg, trg, px, py, u_out, v_out, plain_out) &
                & bind(C, name="spdy_ens_grid_tendencies_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, ug, vg, tg, vorg, divg, trg, px, py, u_out, v_out, plain_out
            integer(c_int), value :: nmem
            integer(c_int) :: rc
        end function
        function spdy_ens_spectral_step_dev(plan, nmem, pvor, pdiv, pspec, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, sdrag, j1, &
                & dt, eps, wil, phi) bind(C, name="spdy_ens_spectral_step_dev") result(rc)
            import :: c_double, c_int, c_ptr
            type(c_ptr), value :: plan, pvor, pdiv, pspec, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, phi
            real(c_double), value :: sdrag, dt, eps, wil
            integer(c_int), value :: nmem, j1
            integer(c_int) :: rc
        end function
        function spdy_ens_direct_batch_spectral_step_dev(plan, nmem, d_ug, d_vg, d_grid, kcos, pvor, pdiv, pspec, vor, div, t, tr, &
                & ps, phis, d_tcorh, d_qcorh, sdrag, j1, dt, eps, wil, phi) &
                & bind(C, name="spdy_ens_direct_batch_spectral_step_dev") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: plan, d_ug, d_vg, d_grid, pvor, pdiv, pspec, vor, div, t, tr, ps, phis, d_tcorh, d_qcorh, phi
            integer(c_int), value :: nmem, kcos, j1
            real(c_double), value :: sdrag, dt, eps, wil
            integer(c_int) :: rc
        end function
        function spdy_ens_geopotential_dev(plan, nmem, t, phis, phi) bind(C, name="spdy_ens_geopotential_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, t, phis, phi
            integer(c_int), value :: nmem
            integer(c_int) :: rc
        end function
        function spdy_ens_physics_workspace(plan, nmem) bind(C, name="spdy_ens_physics_workspace") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), value :: nmem
            integer(c_int) :: rc
        end function
        function spdy_ens_physics_dev(plan, nmem, compute_sw, vor, div, t, q, phi, ps, bnd, albsfc, rad_state, utend, vtend, ttend, &
                & qtend, out) bind(C, name="spdy_ens_physics_dev") result(rc)
            import :: c_int, c_ptr, spdy_sfc_boundary, spdy_column_physics_out
            type(c_ptr), value :: plan, vor, div, t, q, phi, ps, albsfc, rad_state, utend, vtend, ttend, qtend
            integer(c_int), value :: nmem, compute_sw
            type(spdy_sfc_boundary), intent(in) :: bnd
            type(spdy_column_physics_out), intent(in) :: out
            integer(c_int) :: rc
        end function
        ! the surface models (include/spdy.h): this file is one-to-one with the header; the drop-in's own physics still runs on
        ! the host and does not call these
        function spdy_surface_model_create(plan, clim, delt, flags, model) bind(C, name="spdy_surface_model_create") result(rc)
            import :: c_int, c_ptr, c_double, spdy_surface_clim
            type(c_ptr), value :: plan
            type(spdy_surface_clim), intent(in) :: clim
            real(c_double), value :: delt
            integer(c_int), value :: flags
            type(c_ptr), intent(out) :: model
            integer(c_int) :: rc
        end function
        function spdy_ens_surface_model_create(plan, nmem, clim, delt, flags, model) &
                & bind(C, name="spdy_ens_surface_model_create") result(rc)
            import :: c_int, c_ptr, c_double, spdy_surface_clim
            type(c_ptr), value :: plan
            integer(c_int), value :: nmem
            type(spdy_surface_clim), intent(in) :: clim
            real(c_double), value :: delt
            integer(c_int), value :: flags
            type(c_ptr), intent(out) :: model
            integer(c_int) :: rc
        end function
        function spdy_surface_model_members(model, name) bind(C, name="spdy_surface_model_members") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: model, name       ! name: c_loc of a null-terminated string, or c_null_ptr for the object's nmem
            integer(c_int) :: rc
        end function
        function spdy_surface_model_destroy(model) bind(C, name="spdy_surface_model_destroy") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: model
            integer(c_int) :: rc
        end function
        function spdy_surface_model_table(model, name, buf, cap) bind(C, name="spdy_surface_model_table") result(rc)
            import :: c_int, c_ptr, c_char
            type(c_ptr), value :: model, buf
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: cap
            integer(c_int) :: rc
        end function
        function spdy_surface_model_set_date(model, imont1, tmonth, tyear) bind(C, name="spdy_surface_model_set_date") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: model
            integer(c_int), value :: imont1
            real(c_double), value :: tmonth, tyear
            integer(c_int) :: rc
        end function
        function spdy_surface_model_set_sst_anomaly(model, sstan3) bind(C, name="spdy_surface_model_set_sst_anomaly") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: model, sstan3
            integer(c_int) :: rc
        end function
        function spdy_surface_model_couple_dev(model, day, hfluxn, shf, evap, ssrd) bind(C, name="spdy_surface_model_couple_dev") &
                & result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: model, hfluxn, shf, evap, ssrd
            integer(c_int), value :: day
            integer(c_int) :: rc
        end function
        function spdy_surface_model_forcing_dev(model, qcorh) bind(C, name="spdy_surface_model_forcing_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: model, qcorh
            integer(c_int) :: rc
        end function
        function spdy_surface_model_boundary(model, bnd, albsfc) bind(C, name="spdy_surface_model_boundary") result(rc)
            import :: c_int, c_ptr, spdy_sfc_boundary
            type(c_ptr), value :: model
            type(spdy_sfc_boundary), intent(out) :: bnd
            type(c_ptr), intent(out) :: albsfc
            integer(c_int) :: rc
        end function
        function spdy_surface_model_field(model, name, d_ptr) bind(C, name="spdy_surface_model_field") result(rc)
            import :: c_int, c_ptr, c_char
            type(c_ptr), value :: model
            character(kind=c_char), intent(in) :: name(*)
            type(c_ptr), intent(out) :: d_ptr
            integer(c_int) :: rc
        end function
        ! SPPT (include/spdy.h): the pattern object and the column physics with it
        function spdy_sppt_create(plan, nsteps, mu, seed, s) bind(C, name="spdy_sppt_create") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: plan, mu
            integer(c_int), value :: nsteps
            integer(c_long_long), value :: seed
            type(c_ptr), intent(out) :: s
            integer(c_int) :: rc
        end function
        function spdy_sppt_destroy(s) bind(C, name="spdy_sppt_destroy") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: s
            integer(c_int) :: rc
        end function
        function spdy_sppt_reset(s, seed) bind(C, name="spdy_sppt_reset") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: s
            integer(c_long_long), value :: seed
            integer(c_int) :: rc
        end function
        function spdy_sppt_table(s, name, buf, cap) bind(C, name="spdy_sppt_table") result(rc)
            import :: c_int, c_ptr, c_char
            type(c_ptr), value :: s, buf
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: cap
            integer(c_int) :: rc
        end function
        function spdy_sppt_field(s, name, d_ptr) bind(C, name="spdy_sppt_field") result(rc)
            import :: c_int, c_ptr, c_char
            type(c_ptr), value :: s
            character(kind=c_char), intent(in) :: name(*)
            type(c_ptr), intent(out) :: d_ptr
            integer(c_int) :: rc
        end function
        function spdy_sppt_draws(s, draws) bind(C, name="spdy_sppt_draws") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: s
            integer(c_long_long), intent(out) :: draws
            integer(c_int) :: rc
        end function
        function spdy_sppt_advance_dev(s, d_eta) bind(C, name="spdy_sppt_advance_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: s, d_eta
            integer(c_int) :: rc
        end function
        function spdy_column_physics_sppt_workspace(plan) bind(C, name="spdy_column_physics_sppt_workspace") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int) :: rc
        end function
        function spdy_column_physics_sppt_dev(plan, nb, d_pattern, mu, compute_sw, ug, vg, tg, qg, phig, pslg, bnd, albsfc, &
                & rad_state, utend, vtend, ttend, qtend, out) bind(C, name="spdy_column_physics_sppt_dev") result(rc)
            import :: c_int, c_ptr, spdy_sfc_boundary, spdy_column_physics_out
            type(c_ptr), value :: plan, d_pattern, mu, ug, vg, tg, qg, phig, pslg, albsfc, rad_state, utend, vtend, ttend, qtend
            integer(c_int), value :: nb, compute_sw
            type(spdy_sfc_boundary), intent(in) :: bnd
            type(spdy_column_physics_out), intent(in) :: out
            integer(c_int) :: rc
        end function
        function spdy_physics_sppt_workspace(plan) bind(C, name="spdy_physics_sppt_workspace") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int) :: rc
        end function
        function spdy_physics_sppt_dev(plan, s, compute_sw, vor, div, t, q, phi, ps, bnd, albsfc, rad_state, utend, vtend, ttend, &
                & qtend, out) bind(C, name="spdy_physics_sppt_dev") result(rc)
            import :: c_int, c_ptr, spdy_sfc_boundary, spdy_column_physics_out
            type(c_ptr), value :: plan, s, vor, div, t, q, phi, ps, albsfc, rad_state, utend, vtend, ttend, qtend
            integer(c_int), value :: compute_sw
            type(spdy_sfc_boundary), intent(in) :: bnd
            type(spdy_column_physics_out), intent(in) :: out
            integer(c_int) :: rc
        end function
        ! the ensemble form: nmem patterns in one object (seeds: nmem 64-bit values on the host), one advance for all members
        function spdy_ens_sppt_create(plan, nmem, nsteps, mu, seeds, s) bind(C, name="spdy_ens_sppt_create") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, mu, seeds
            integer(c_int), value :: nmem, nsteps
            type(c_ptr), intent(out) :: s
            integer(c_int) :: rc
        end function
        function spdy_sppt_members(s) bind(C, name="spdy_sppt_members") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: s
            integer(c_int) :: rc
        end function
        function spdy_ens_sppt_reset(s, member, seed) bind(C, name="spdy_ens_sppt_reset") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: s
            integer(c_int), value :: member
            integer(c_long_long), value :: seed
            integer(c_int) :: rc
        end function
        function spdy_ens_sppt_draws(s, member, draws) bind(C, name="spdy_ens_sppt_draws") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: s
            integer(c_int), value :: member
            integer(c_long_long), intent(out) :: draws
            integer(c_int) :: rc
        end function
        function spdy_ens_physics_sppt_workspace(plan, nmem) bind(C, name="spdy_ens_physics_sppt_workspace") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), value :: nmem
            integer(c_int) :: rc
        end function
        function spdy_ens_physics_sppt_dev(plan, nmem, s, compute_sw, vor, div, t, q, phi, ps, bnd, albsfc, rad_state, utend, vtend, &
                & ttend, qtend, out) bind(C, name="spdy_ens_physics_sppt_dev") result(rc)
            import :: c_int, c_ptr, spdy_sfc_boundary, spdy_column_physics_out
            type(c_ptr), value :: plan, s, vor, div, t, q, phi, ps, albsfc, rad_state, utend, vtend, ttend, qtend
            integer(c_int), value :: nmem, compute_sw
            type(spdy_sfc_boundary), intent(in) :: bnd
            type(spdy_column_physics_out), intent(in) :: out
            integer(c_int) :: rc
        end function
        ! diagnostics (include/spdy.h): check_diagnostics on the device, the history ring and the sticky stop flag
        function spdy_diagnostics_create(plan, capacity, first_step, d) bind(C, name="spdy_diagnostics_create") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: plan
            integer(c_int), value :: capacity
            integer(c_long_long), value :: first_step
            type(c_ptr), intent(out) :: d
            integer(c_int) :: rc
        end function
        function spdy_ens_diagnostics_create(plan, nmem, capacity, first_step, d) bind(C, name="spdy_ens_diagnostics_create") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: plan
            integer(c_int), value :: nmem, capacity
            integer(c_long_long), value :: first_step
            type(c_ptr), intent(out) :: d
            integer(c_int) :: rc
        end function
        function spdy_ens_diagnostics_status(d, member, next_step, bad_step, bad_level, bad_mask, bad_row) &
                & bind(C, name="spdy_ens_diagnostics_status") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: d, bad_row
            integer(c_int), value :: member
            integer(c_long_long), intent(out) :: next_step, bad_step
            integer(c_int), intent(out) :: bad_level, bad_mask
            integer(c_int) :: rc
        end function
        function spdy_ens_diagnostics_read(d, member, step, count, rows) bind(C, name="spdy_ens_diagnostics_read") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: d, rows
            integer(c_int), value :: member, count
            integer(c_long_long), value :: step
            integer(c_int) :: rc
        end function
        function spdy_ens_diagnostics_stopped(d, bad_step) bind(C, name="spdy_ens_diagnostics_stopped") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: d
            integer(c_long_long), intent(out) :: bad_step(*)
            integer(c_int) :: rc
        end function
        function spdy_diagnostics_destroy(d) bind(C, name="spdy_diagnostics_destroy") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: d
            integer(c_int) :: rc
        end function
        function spdy_diagnostics_set_limits(d, limits) bind(C, name="spdy_diagnostics_set_limits") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: d, limits
            integer(c_int) :: rc
        end function
        function spdy_diagnostics_reset(d, next_step) bind(C, name="spdy_diagnostics_reset") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: d
            integer(c_long_long), value :: next_step
            integer(c_int) :: rc
        end function
        function spdy_diagnostics_check_dev(d, vor, div, t) bind(C, name="spdy_diagnostics_check_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: d, vor, div, t
            integer(c_int) :: rc
        end function
        function spdy_diagnostics_status(d, next_step, bad_step, bad_level, bad_mask, bad_row) &
                & bind(C, name="spdy_diagnostics_status") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: d, bad_row
            integer(c_long_long), intent(out) :: next_step, bad_step
            integer(c_int), intent(out) :: bad_level, bad_mask
            integer(c_int) :: rc
        end function
        function spdy_diagnostics_read(d, step, count, rows) bind(C, name="spdy_diagnostics_read") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: d, rows
            integer(c_long_long), value :: step
            integer(c_int), value :: count
            integer(c_int) :: rc
        end function
        function spdy_diagnostics_field(d, name, d_ptr) bind(C, name="spdy_diagnostics_field") result(rc)
            import :: c_int, c_ptr, c_char
            type(c_ptr), value :: d
            character(kind=c_char), intent(in) :: name(*)
            type(c_ptr), intent(out) :: d_ptr
            integer(c_int) :: rc
        end function
        function spdy_diagnostics_format(kx, step, row, buf, cap) bind(C, name="spdy_diagnostics_format") result(rc)
            import :: c_int, c_ptr, c_long_long, c_char
            integer(c_int), value :: kx, cap
            integer(c_long_long), value :: step
            type(c_ptr), value :: row
            character(kind=c_char), intent(inout) :: buf(*)
            integer(c_int) :: rc
        end function
        function spdy_output_workspace(plan) bind(C, name="spdy_output_workspace") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int) :: rc
        end function
        function spdy_output_batch_dev(plan, vor, div, t, q, phi, ps, u_out, v_out, t_out, q_out, phi_out, ps_out) &
                & bind(C, name="spdy_output_batch_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, vor, div, t, q, phi, ps, u_out, v_out, t_out, q_out, phi_out, ps_out
            integer(c_int) :: rc
        end function
        ! the ensemble output (include/spdy.h): members, mean, spread are c_loc of a spdy_output_fields, or c_null_ptr = not wanted;
        ! d_use is a device array of nmem c_int, or c_null_ptr = all members
        function spdy_ens_output_workspace(plan, nmem) bind(C, name="spdy_ens_output_workspace") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), value :: nmem
            integer(c_int) :: rc
        end function
        function spdy_ens_output_batch_dev(plan, nmem, vor, div, t, q, phi, ps, d_use, members, mean, spread) &
                & bind(C, name="spdy_ens_output_batch_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, vor, div, t, q, phi, ps, d_use, members, mean, spread
            integer(c_int), value :: nmem
            integer(c_int) :: rc
        end function
        ! the pressure-level output (include/spdy.h): plev is c_loc of nlev c_double on the HOST, in Pa; coord is SPDY_PLEV_LINEAR_P
        ! or SPDY_PLEV_LOG_P; below is a device array of c_float (ix,il,nlev), or c_null_ptr = not wanted; the groups as above
        function spdy_ens_output_pressure_dev(plan, nmem, vor, div, t, q, phi, ps, d_use, nlev, plev, coord, members, mean, spread, &
                & below) bind(C, name="spdy_ens_output_pressure_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, vor, div, t, q, phi, ps, d_use, plev, members, mean, spread, below
            integer(c_int), value :: nmem, nlev, coord
            integer(c_int) :: rc
        end function
        function spdy_ens_output_pressure_grid_dev(plan, nmem, grid, d_use, nlev, plev, coord, members, mean, spread, below) &
                & bind(C, name="spdy_ens_output_pressure_grid_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, grid, d_use, plev, members, mean, spread, below
            integer(c_int), value :: nmem, nlev, coord
            integer(c_int) :: rc
        end function
        function spdy_output_pressure_dev(plan, vor, div, t, q, phi, ps, nlev, plev, coord, u_out, v_out, t_out, q_out, phi_out, &
                & ps_out) bind(C, name="spdy_output_pressure_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan, vor, div, t, q, phi, ps, plev, u_out, v_out, t_out, q_out, phi_out, ps_out
            integer(c_int), value :: nlev, coord
            integer(c_int) :: rc
        end function
        ! the ensemble analysis (include/spdy.h): host is c_loc of an array of spdy_obs; the device pointers are those of time
        ! level 1 of the ensemble (spdy_ens_letkf_dev) or of a gridded ensemble (spdy_letkf_analyse_grid_dev)
        function spdy_letkf_create(plan, nmem, max_obs, l) bind(C, name="spdy_letkf_create") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: plan
            integer(c_int), value :: nmem, max_obs
            type(c_ptr), intent(out) :: l
            integer(c_int) :: rc
        end function
        function spdy_letkf_destroy(l) bind(C, name="spdy_letkf_destroy") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l
            integer(c_int) :: rc
        end function
        function spdy_letkf_set_localization(l, sigma_h_m, sigma_v_lnsigma, rho) bind(C, name="spdy_letkf_set_localization") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: l
            real(c_double), value :: sigma_h_m, sigma_v_lnsigma, rho
            integer(c_int) :: rc
        end function
        function spdy_letkf_set_obs(l, nobs, host) bind(C, name="spdy_letkf_set_obs") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l, host
            integer(c_int), value :: nobs
            integer(c_int) :: rc
        end function
        ! host is c_loc of an array of spdy_pobs: observations that may be given at a pressure (lev = SPDY_OBS_AT_P, p in Pa)
        function spdy_pobs_set(l, nobs, host) bind(C, name="spdy_pobs_set") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l, host
            integer(c_int), value :: nobs
            integer(c_int) :: rc
        end function
        function spdy_letkf_set_weight_stride(l, si, sj) bind(C, name="spdy_letkf_set_weight_stride") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l
            integer(c_int), value :: si, sj
            integer(c_int) :: rc
        end function
        ! relaxation to the prior perturbations (rtpp) and spread (rtps), both in [0, 1]; (0, 0): none
        function spdy_relax_set(l, rtpp, rtps) bind(C, name="spdy_relax_set") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: l
            real(c_double), value :: rtpp, rtps
            integer(c_int) :: rc
        end function
        ! observations in time slots (include/spdy.h, "observations in time slots"): first is c_loc of nslots + 1 integers
        function spdy_slot_set(l, nslots, first) bind(C, name="spdy_slot_set") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l, first
            integer(c_int), value :: nslots
            integer(c_int) :: rc
        end function
        function spdy_slot_observe_grid_dev(l, slot, ug, vg, tg, qg, psg) bind(C, name="spdy_slot_observe_grid_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l, ug, vg, tg, qg, psg
            integer(c_int), value :: slot
            integer(c_int) :: rc
        end function
        function spdy_slot_observe_dev(l, slot, vor, div, t, q, ps) bind(C, name="spdy_slot_observe_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l, vor, div, t, q, ps
            integer(c_int), value :: slot
            integer(c_int) :: rc
        end function
        function spdy_slot_analyse_grid_dev(l, ug, vg, tg, qg, psg, du, dv, dt, dq, dps, d_use) &
                & bind(C, name="spdy_slot_analyse_grid_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l, ug, vg, tg, qg, psg, du, dv, dt, dq, dps, d_use
            integer(c_int) :: rc
        end function
        function spdy_slot_ens_letkf_dev(l, vor, div, t, q, ps, d_use) bind(C, name="spdy_slot_ens_letkf_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l, vor, div, t, q, ps, d_use
            integer(c_int) :: rc
        end function
        function spdy_slot_nature_observe_dev(n, letkf, slot, noise) bind(C, name="spdy_slot_nature_observe_dev") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: n, letkf
            integer(c_int), value :: slot
            real(c_double), value :: noise
            integer(c_int) :: rc
        end function
        ! background check and observation statistics (include/spdy.h): group is c_null_ptr (the default grouping, the
        ! observation's variable) or c_loc of nobs integers in [0, ngroups)
        function spdy_qc_set(l, gross, ngroups, group) bind(C, name="spdy_qc_set") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: l, group
            real(c_double), value :: gross
            integer(c_int), value :: ngroups
            integer(c_int) :: rc
        end function
        function spdy_qc_set_slot(l, slot) bind(C, name="spdy_qc_set_slot") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l
            integer(c_int), value :: slot
            integer(c_int) :: rc
        end function
        function spdy_qc_stats_grid_dev(l, ug, vg, tg, qg, psg, d_use, slot) bind(C, name="spdy_qc_stats_grid_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l, ug, vg, tg, qg, psg, d_use
            integer(c_int), value :: slot
            integer(c_int) :: rc
        end function
        function spdy_qc_stats_dev(l, vor, div, t, q, ps, d_use, slot) bind(C, name="spdy_qc_stats_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l, vor, div, t, q, ps, d_use
            integer(c_int), value :: slot
            integer(c_int) :: rc
        end function
        ! adaptive inflation (include/spdy.h): on /= 0 switches the field rho[kx][ncol] on in the scalar rho's place
        function spdy_infl_set(l, on, sigma_b, rho_min, rho_max) bind(C, name="spdy_infl_set") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: l
            integer(c_int), value :: on
            real(c_double), value :: sigma_b, rho_min, rho_max
            integer(c_int) :: rc
        end function
        function spdy_infl_fill(l, rho0) bind(C, name="spdy_infl_fill") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: l
            real(c_double), value :: rho0
            integer(c_int) :: rc
        end function
        function spdy_letkf_table(l, name, buf, cap) bind(C, name="spdy_letkf_table") result(rc)
            import :: c_int, c_ptr, c_char
            type(c_ptr), value :: l, buf
            character(kind=c_char), intent(in) :: name(*)
            integer(c_int), value :: cap
            integer(c_int) :: rc
        end function
        function spdy_letkf_field(l, name, d_ptr) bind(C, name="spdy_letkf_field") result(rc)
            import :: c_int, c_ptr, c_char
            type(c_ptr), value :: l
            character(kind=c_char), intent(in) :: name(*)
            type(c_ptr), intent(out) :: d_ptr
            integer(c_int) :: rc
        end function
        function spdy_letkf_analyse_grid_dev(l, ug, vg, tg, qg, psg, du, dv, dt, dq, dps) &
                & bind(C, name="spdy_letkf_analyse_grid_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l, ug, vg, tg, qg, psg, du, dv, dt, dq, dps
            integer(c_int) :: rc
        end function
        function spdy_ens_letkf_dev(l, vor, div, t, q, ps) bind(C, name="spdy_ens_letkf_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l, vor, div, t, q, ps
            integer(c_int) :: rc
        end function
        ! the member mask (include/spdy.h): d_use is nmem C ints in device memory, non-zero = the member is in use, read when
        ! the kernels run; c_null_ptr = all members.  The analysis and the scores over the members in use, and the guard's
        ! sticky records as such a mask
        function spdy_mask_letkf_analyse_grid_dev(l, ug, vg, tg, qg, psg, du, dv, dt, dq, dps, d_use) &
                & bind(C, name="spdy_mask_letkf_analyse_grid_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l, ug, vg, tg, qg, psg, du, dv, dt, dq, dps, d_use
            integer(c_int) :: rc
        end function
        function spdy_mask_ens_letkf_dev(l, vor, div, t, q, ps, d_use) bind(C, name="spdy_mask_ens_letkf_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: l, vor, div, t, q, ps, d_use
            integer(c_int) :: rc
        end function
        function spdy_mask_nature_verify_dev(n, letkf, vor, div, t, q, ps, d_use, slot) &
                & bind(C, name="spdy_mask_nature_verify_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: n, letkf, vor, div, t, q, ps, d_use
            integer(c_int), value :: slot
            integer(c_int) :: rc
        end function
        function spdy_mask_nature_verify_grid_dev(n, nmem, ug, vg, tg, qg, psg, d_use, slot) &
                & bind(C, name="spdy_mask_nature_verify_grid_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: n, ug, vg, tg, qg, psg, d_use
            integer(c_int), value :: nmem, slot
            integer(c_int) :: rc
        end function
        function spdy_mask_from_diagnostics_dev(d, d_use) bind(C, name="spdy_mask_from_diagnostics_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: d, d_use
            integer(c_int) :: rc
        end function
        ! the nature run (include/spdy.h): the truth of a twin experiment, the observation values of an analysis object's network
        ! drawn from it, an ensemble's scores against it; the device pointers are those of time level 1
        function spdy_nature_create(plan, seed, capacity, n) bind(C, name="spdy_nature_create") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: plan
            integer(c_long_long), value :: seed
            integer(c_int), value :: capacity
            type(c_ptr), intent(out) :: n
            integer(c_int) :: rc
        end function
        function spdy_nature_destroy(n) bind(C, name="spdy_nature_destroy") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: n
            integer(c_int) :: rc
        end function
        function spdy_nature_reset(n, seed) bind(C, name="spdy_nature_reset") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: n
            integer(c_long_long), value :: seed
            integer(c_int) :: rc
        end function
        function spdy_nature_draws(n, count) bind(C, name="spdy_nature_draws") result(rc)
            import :: c_int, c_ptr, c_long_long
            type(c_ptr), value :: n
            integer(c_long_long), intent(out) :: count
            integer(c_int) :: rc
        end function
        function spdy_nature_field(n, name, d_ptr) bind(C, name="spdy_nature_field") result(rc)
            import :: c_int, c_ptr, c_char
            type(c_ptr), value :: n
            character(kind=c_char), intent(in) :: name(*)
            type(c_ptr), intent(out) :: d_ptr
            integer(c_int) :: rc
        end function
        function spdy_nature_set_state_dev(n, vor, div, t, q, ps) bind(C, name="spdy_nature_set_state_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: n, vor, div, t, q, ps
            integer(c_int) :: rc
        end function
        function spdy_nature_observe_dev(n, letkf, noise) bind(C, name="spdy_nature_observe_dev") result(rc)
            import :: c_int, c_ptr, c_double
            type(c_ptr), value :: n, letkf
            real(c_double), value :: noise
            integer(c_int) :: rc
        end function
        function spdy_nature_verify_dev(n, letkf, vor, div, t, q, ps, slot) bind(C, name="spdy_nature_verify_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: n, letkf, vor, div, t, q, ps
            integer(c_int), value :: slot
            integer(c_int) :: rc
        end function
        function spdy_nature_verify_grid_dev(n, nmem, ug, vg, tg, qg, psg, slot) bind(C, name="spdy_nature_verify_grid_dev") result(rc)
            import :: c_int, c_ptr
            type(c_ptr), value :: n, ug, vg, tg, qg, psg
            integer(c_int), value :: nmem, slot
            integer(c_int) :: rc
        end function
    end interface

    integer(c_int), parameter :: SPDY_OBS_U = 0_c_int, SPDY_OBS_V = 1_c_int, SPDY_OBS_T = 2_c_int, SPDY_OBS_Q = 3_c_int, &
        & SPDY_OBS_PS = 4_c_int                                !! spdy_obs%var (include/spdy.h)
    integer(c_int), parameter :: SPDY_MAX_SLOTS = 32_c_int     !! the most time slots of spdy_slot_set (include/spdy.h)
    integer(c_int), parameter :: SPDY_QC_MAX_GROUPS = 64_c_int, SPDY_QC_SLOTS = 4_c_int
                                                               !! background check: the most groups, the statistics' rows (include/spdy.h)
    integer(c_int), parameter :: SPDY_OBS_AT_P = -1_c_int      !! spdy_pobs%lev: the observation sits at p (include/spdy.h)
    integer(c_int), parameter :: SPDY_DEVICE_AUTO = -2_c_int   !! $SPDY_DEVICE, else the launcher's local rank (include/spdy.h)
    integer(c_int), parameter :: SPDY_MAX_PLEV = 32_c_int, SPDY_PLEV_LINEAR_P = 0_c_int, SPDY_PLEV_LOG_P = 1_c_int
                                                               !! pressure-level output: the level count's bound, coord (include/spdy.h)

    !> Work a drop-in module has deferred on the device and that must be issued before the plan's tables change (time_stepping's
    !  collected leapfrog steps under steps_per_launch > 1): the module registers its flush routine here, and every wrapper that
    !  re-uploads tables (implicit%initialize_implicit) calls spdy_flush_pending first -- no circular module dependency.
    abstract interface
        subroutine spdy_flush_iface()
        end subroutine
    end interface
    procedure(spdy_flush_iface), pointer, save :: spdy_pending_flush => null()

contains
    subroutine spdy_flush_pending()
        if (associated(spdy_pending_flush)) call spdy_pending_flush()
    end subroutine

    !> The reference has no status returns (it `stop`s on fatal errors, e.g. matrix_inversion.f90:26);
    !  the drop-in keeps the signatures and turns a non-zero C status into `error stop`.
    subroutine spdy_check(rc, what)
        integer(c_int), intent(in) :: rc
        character(*), intent(in) :: what
        character(kind=c_char), pointer :: msg(:)
        type(c_ptr) :: cmsg
        integer :: n
        if (rc >= 0) return
        cmsg = spdy_last_error()
        call c_f_pointer(cmsg, msg, [512])
        n = 0
        do while (n < 512)
            if (msg(n + 1) == c_null_char) exit
            n = n + 1
        end do
        write (*, '(3A,I0,2A)') 'spdy: ', what, ' failed (', rc, '): ', transfer(msg(1:n), repeat(' ', n))
        error stop 'spdy: HIP spectral-transform path failed'
    end subroutine
end module

! radar_shims.F90 -- the front end of the radar simulator of GEOSsatsim_GridComp's COSP for a Fortran caller; the bodies call the C ABI of
! include/geosrad_radar.h.
!   prec_scops             an external subroutine with the reference's own name and argument list (llnl/prec_scops.f:25-26).  The
!                          reference's is a Fortran 77 routine that cosp.F90:411 calls without an interface, so this is a true drop-in:
!                          leave llnl/prec_scops.f out of the build and link this.
!   geosrad_cosp_sghydro   module geosrad_radar: a batched call for the sub-grid hydrometeor block of cosp_iter (cosp.F90:399-519 with
!                          use_precipitation_fluxes = .false.), which is inline in the reference and has no routine to replace
!   geosrad_radar_gases    module geosrad_radar: gases() for every volume and path_integral() to every gate (radar_simulator.f90:470-484),
!                          which the reference evaluates inside radar_simulator's loops
! These are the host-array entry points (one round trip over PCIe a call, chunked by geosrad_set_chunk); the `_dev` variants take device
! pointers and the byte mask geosrad_scops_dev leaves (INTEGRATION.md).
module geosrad_radar_c
   use iso_c_binding
   implicit none
   interface
      integer(c_int) function geosrad_prec_scops_c(ctx, npoints, nlev, ncol, ls_p_rate, cv_p_rate, frac_out, prec_frac) &
            bind(C, name='geosrad_prec_scops')
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx, ls_p_rate, cv_p_rate, frac_out, prec_frac
         integer(c_int), value :: npoints, nlev, ncol
      end function
      integer(c_int) function geosrad_cosp_sghydro_c(ctx, npoints, nlev, ncol, frac_out, mr_lsliq, mr_lsice, mr_lsrain, mr_lssnow, mr_cvliq, &
            mr_cvice, mr_cvrain, mr_cvsnow, mr_lsgrpl, prec_frac, frac_ls, frac_cv, prec_ls, prec_cv, mr_sub, mr_hydro_sg) &
            bind(C, name='geosrad_cosp_sghydro')
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx, frac_out, mr_lsliq, mr_lsice, mr_lsrain, mr_lssnow, mr_cvliq, mr_cvice, mr_cvrain, mr_cvsnow, mr_lsgrpl, &
            prec_frac, frac_ls, frac_cv, prec_ls, prec_cv, mr_sub, mr_hydro_sg
         integer(c_int), value :: npoints, nlev, ncol
      end function
      integer(c_int) function geosrad_radar_gases_c(ctx, npoints, nlev, p, t, rh, zlev, freq, surface_radar, g_vol, g_to_vol) &
            bind(C, name='geosrad_radar_gases')
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: ctx, p, t, rh, zlev, g_vol, g_to_vol
         integer(c_int), value :: npoints, nlev, surface_radar
         real(c_double), value :: freq
      end function
   end interface
   ! the last index of mr_hydro / mr_sub: the I_* of cosp_constants.F90:39-47 (the GEOSRAD_HYDRO_* of include/geosrad_radar.h plus one)
   integer, parameter :: GEOSRAD_HYDRO_LSLIQ = 1, GEOSRAD_HYDRO_LSICE = 2, GEOSRAD_HYDRO_LSRAIN = 3, GEOSRAD_HYDRO_LSSNOW = 4, &
      GEOSRAD_HYDRO_CVLIQ = 5, GEOSRAD_HYDRO_CVICE = 6, GEOSRAD_HYDRO_CVRAIN = 7, GEOSRAD_HYDRO_CVSNOW = 8, GEOSRAD_HYDRO_LSGRPL = 9, &
      GEOSRAD_NHYDRO = 9
end module geosrad_radar_c

module geosrad_radar
   use iso_c_binding
   implicit none
contains
   ! frac_out (npoints,ncol,nlev) the real mask of scops, level 1 the top; mr_hydro (npoints,nlev,9) the gridbox mixing ratios in the I_*
   ! order, level 1 the top (gbx%mr_hydro counts from the surface: hand over mr_hydro(:,nlev:1:-1,:)).  prec_frac (npoints,ncol,nlev);
   ! frac_ls, frac_cv, prec_ls, prec_cv (npoints,nlev); mr_sub (npoints,nlev,9): what a sub-column of the matching kind carries.
   subroutine geosrad_cosp_sghydro(npoints, nlev, ncol, frac_out, mr_hydro, prec_frac, frac_ls, frac_cv, prec_ls, prec_cv, mr_sub)
      use geosrad_c, only: geosrad_ctx_handle, geosrad_fail
      use geosrad_radar_c, only: geosrad_cosp_sghydro_c
      integer, intent(in) :: npoints, nlev, ncol
      real, target, intent(in) :: frac_out(npoints,ncol,nlev), mr_hydro(npoints,nlev,9)
      real, target, intent(out) :: prec_frac(npoints,ncol,nlev), frac_ls(npoints,nlev), frac_cv(npoints,nlev), prec_ls(npoints,nlev), &
         prec_cv(npoints,nlev), mr_sub(npoints,nlev,9)
      integer(c_int) :: rc
      rc = geosrad_cosp_sghydro_c(geosrad_ctx_handle(), int(npoints,c_int), int(nlev,c_int), int(ncol,c_int), c_loc(frac_out), &
         c_loc(mr_hydro(:,:,1)), c_loc(mr_hydro(:,:,2)), c_loc(mr_hydro(:,:,3)), c_loc(mr_hydro(:,:,4)), c_loc(mr_hydro(:,:,5)), &
         c_loc(mr_hydro(:,:,6)), c_loc(mr_hydro(:,:,7)), c_loc(mr_hydro(:,:,8)), c_loc(mr_hydro(:,:,9)), c_loc(prec_frac), c_loc(frac_ls), &
         c_loc(frac_cv), c_loc(prec_ls), c_loc(prec_cv), c_loc(mr_sub), c_null_ptr)
      if (rc /= 0) call geosrad_fail('geosrad_cosp_sghydro')
   end subroutine geosrad_cosp_sghydro

   ! p (Pa), t (K), rh (%), zlev (m) (npoints,nlev), level 1 the top; freq GHz; surface_radar 0 spaceborne, 1 at the surface.  g_vol dB/km
   ! and g_to_vol dB (npoints,nlev), real(8) in either build, as quickbeam holds them.
   subroutine geosrad_radar_gases(npoints, nlev, p, t, rh, zlev, freq, surface_radar, g_vol, g_to_vol)
      use geosrad_c, only: geosrad_ctx_handle, geosrad_fail
      use geosrad_radar_c, only: geosrad_radar_gases_c
      integer, intent(in) :: npoints, nlev, surface_radar
      real, target, intent(in) :: p(npoints,nlev), t(npoints,nlev), rh(npoints,nlev), zlev(npoints,nlev)
      real(8), intent(in) :: freq
      real(8), target, intent(out) :: g_vol(npoints,nlev), g_to_vol(npoints,nlev)
      integer(c_int) :: rc
      rc = geosrad_radar_gases_c(geosrad_ctx_handle(), int(npoints,c_int), int(nlev,c_int), c_loc(p), c_loc(t), c_loc(rh), c_loc(zlev), &
         real(freq,c_double), int(surface_radar,c_int), c_loc(g_vol), c_loc(g_to_vol))
      if (rc /= 0) call geosrad_fail('geosrad_radar_gases')
   end subroutine geosrad_radar_gases
end module geosrad_radar

subroutine prec_scops(npoints, nlev, ncol, ls_p_rate, cv_p_rate, frac_out, prec_frac)
   use iso_c_binding
   use geosrad_c, only: geosrad_ctx_handle, geosrad_fail
   use geosrad_radar_c, only: geosrad_prec_scops_c
   implicit none
   integer npoints, nlev, ncol
   real, target :: ls_p_rate(npoints,nlev), cv_p_rate(npoints,nlev)
   real, target :: frac_out(npoints,ncol,nlev), prec_frac(npoints,ncol,nlev)
   integer(c_int) :: rc
   rc = geosrad_prec_scops_c(geosrad_ctx_handle(), int(npoints,c_int), int(nlev,c_int), int(ncol,c_int), c_loc(ls_p_rate), c_loc(cv_p_rate), &
      c_loc(frac_out), c_loc(prec_frac))
   if (rc /= 0) call geosrad_fail('prec_scops')
end subroutine prec_scops

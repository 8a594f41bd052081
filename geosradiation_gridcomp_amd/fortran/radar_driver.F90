! radar_driver.F90 -- a caller of the drop-in external `prec_scops` and of the batched `geosrad_cosp_sghydro` and `geosrad_radar_gases` of
! module geosrad_radar (radar_shims.F90): prec_scops without an interface block, the way cosp.F90:411 calls it, on the rates
! cosp.F90:404-408 forms; explicit-shape arrays from the top of the atmosphere down.
! Reads npoints, nlev, ncol, surface_radar (integers), freq (real(8)), then frac_out (npoints,ncol,nlev), the nine mixing ratios
! (npoints,nlev,9) and p, t, rh, zlev (npoints,nlev) as real(4), written by tests/test_fortran_radar_inputs.py; writes every result as
! real(8) in the order of the `write` statements below.
program radar_driver
   use geosrad_radar, only: geosrad_cosp_sghydro, geosrad_radar_gases
   use geosrad_radar_c, only: GEOSRAD_HYDRO_LSRAIN, GEOSRAD_HYDRO_LSSNOW, GEOSRAD_HYDRO_LSGRPL, GEOSRAD_HYDRO_CVRAIN, GEOSRAD_HYDRO_CVSNOW
   implicit none
   integer :: npoints, nlev, ncol, surface_radar, u, k
   real(8) :: freq
   real(4), allocatable :: b3(:,:,:), b2(:,:)
   real, allocatable :: frac_out(:,:,:), mr(:,:,:), a(:,:,:), ls_p_rate(:,:), cv_p_rate(:,:), prec_frac(:,:,:), prec2(:,:,:)
   real, allocatable :: frac_ls(:,:), frac_cv(:,:), prec_ls(:,:), prec_cv(:,:), mr_sub(:,:,:)
   real(8), allocatable :: g_vol(:,:), g_to_vol(:,:)
   character(len=512) :: fi, fo
   call get_command_argument(1, fi); call get_command_argument(2, fo)
   open(newunit=u, file=trim(fi), access='stream', form='unformatted', status='old')
   read(u) npoints, nlev, ncol, surface_radar, freq
   allocate(b3(npoints,ncol,nlev), b2(npoints,nlev), frac_out(npoints,ncol,nlev), mr(npoints,nlev,9), a(npoints,nlev,4))
   read(u) b3; frac_out = b3
   do k = 1, 9
      read(u) b2; mr(:,:,k) = b2
   end do
   do k = 1, 4
      read(u) b2; a(:,:,k) = b2
   end do
   close(u)
   allocate(ls_p_rate(npoints,nlev), cv_p_rate(npoints,nlev), prec_frac(npoints,ncol,nlev), prec2(npoints,ncol,nlev))
   allocate(frac_ls(npoints,nlev), frac_cv(npoints,nlev), prec_ls(npoints,nlev), prec_cv(npoints,nlev), mr_sub(npoints,nlev,9))
   allocate(g_vol(npoints,nlev), g_to_vol(npoints,nlev))
   open(newunit=u, file=trim(fo), access='stream', form='unformatted', status='replace')

   ls_p_rate = mr(:,:,GEOSRAD_HYDRO_LSRAIN) + mr(:,:,GEOSRAD_HYDRO_LSSNOW) + mr(:,:,GEOSRAD_HYDRO_LSGRPL)
   cv_p_rate = mr(:,:,GEOSRAD_HYDRO_CVRAIN) + mr(:,:,GEOSRAD_HYDRO_CVSNOW)
   call prec_scops(npoints,nlev,ncol,ls_p_rate,cv_p_rate,frac_out,prec_frac)
   write(u) real(prec_frac, 8)

   call geosrad_cosp_sghydro(npoints,nlev,ncol,frac_out,mr,prec2,frac_ls,frac_cv,prec_ls,prec_cv,mr_sub)
   write(u) real(prec2, 8), real(frac_ls, 8), real(frac_cv, 8), real(prec_ls, 8), real(prec_cv, 8), real(mr_sub, 8)

   call geosrad_radar_gases(npoints,nlev,a(:,:,1),a(:,:,2),a(:,:,3),a(:,:,4),freq,surface_radar,g_vol,g_to_vol)
   write(u) g_vol, g_to_vol
   close(u)
end program radar_driver

! lwchou_driver.F90 -- the Chou-Suarez branch of LW_Driver as GEOS_IrradGridComp would run it with its fields on the device
! (GEOS_IrradGridComp.F90:1781-1785, :1876-1912, :2093-2108, :3604-3663): GEOS-native fields in (model ordering, Pa, radii in metres with
! MAPL_UNDEF cells), `call lw_driver_chou`, the INTERNAL fluxes and the refresh-time exports out.  Reads a batch written by
! tests/test_gpu_lw_chou_driver.py (fields in LWK_* order; have_aer = 0: no aerosol provider, the three arrays are absent), writes
! FLXU_INT, FLXD_INT, DFDTS, FLX_INT, SFCEM_INT, TAUIR, CLDTMP, CLDPRS, LWS0.
program lwchou_driver
   use iso_c_binding
   use geosrad_gridcomp
   implicit none
   integer :: ncol, lm, lcldmh, lcldlm, have_aer, binary, u, k, rc, n3, n3p, nin
   integer :: sz(LWK_NIN)
   real(8) :: consts(LWK_NCONST)
   real(4), allocatable :: buf(:)
   real, allocatable :: a(:), o3p(:,:), o3(:), o2(:,:)
   type(c_ptr) :: fin(LWK_NIN), fout(LWK_NOUT)
   integer, parameter :: w3p(4) = [LWK_FLXU_INT, LWK_FLXD_INT, LWK_DFDTS, LWK_FLX_INT], w2(4) = [LWK_SFCEM_INT, LWK_CLDTMP, LWK_CLDPRS, LWK_LWS0]
   character(len=512) :: fi, fo
   call get_command_argument(1, fi); call get_command_argument(2, fo)
   open(newunit=u, file=trim(fi), access='stream', form='unformatted', status='old')
   read(u) ncol, lm, lcldmh, lcldlm, have_aer, binary
   read(u) consts
   n3 = ncol * lm; n3p = ncol * (lm + 1)
   sz = n3
   sz(LWK_PLE) = n3p
   sz([LWK_TS, LWK_EMIS]) = ncol
   sz([LWK_TAUA, LWK_SSAA, LWK_ASYA]) = n3 * 10
   nin = merge(LWK_NIN, LWK_EMIS, have_aer /= 0)
   fin = c_null_ptr
   do k = 1, nin
      allocate(buf(sz(k)), a(sz(k))); read(u) buf; a = real(buf, kind(a))
      fin(k) = dev_alloc(sz(k)); call dev_put(fin(k), a, sz(k))
      deallocate(buf, a)
   end do
   close(u)
   fout = c_null_ptr
   do k = LWK_FLXU_INT, LWK_DFDTS
      fout(k) = dev_alloc(n3p)
   end do
   fout(LWK_FLX_INT) = dev_alloc(n3p); fout(LWK_TAUIR) = dev_alloc(n3)
   do k = 1, 4
      fout(w2(k)) = dev_alloc(ncol)
   end do
   call lw_driver_chou(ncol, lm, fin, consts, .true., lcldmh, lcldlm, binary /= 0, fout, rc)
   if (rc /= 0) error stop 'lw_driver_chou failed'
   call dev_sync()
   allocate(o3p(n3p, 4), o3(n3), o2(ncol, 4))
   do k = 1, 4
      call dev_get(o3p(:, k), fout(w3p(k)), n3p); call dev_get(o2(:, k), fout(w2(k)), ncol)
   end do
   call dev_get(o3, fout(LWK_TAUIR), n3)
   open(newunit=u, file=trim(fo), access='stream', form='unformatted', status='replace')
   write(u) real(o3p,8), real(o2(:,1),8), real(o3,8), real(o2(:,2:4),8)
   close(u)
   do k = 1, LWK_NIN
      if (c_associated(fin(k))) call dev_free(fin(k))
   end do
   do k = 1, LWK_NOUT
      if (c_associated(fout(k))) call dev_free(fout(k))
   end do
end program lwchou_driver

! swclouds_driver.F90 -- the cloud diagnostics of UPDATE_EXPORT as GEOS_SolarGridComp would run them every model step with its fields on the
! device (GEOS_SolarGridComp.F90:7006-7058, :7223-7392): FCLD, PLE, T, QI..QS, RI..RS, ZTH in, `call sw_update_clouds`, every export
! out.  Reads a batch written by tests/test_sw_clouds.py (fields in SWK_* order), writes the exports in SWK_* order as real(8).
program swclouds_driver
   use iso_c_binding
   use geosrad_gridcomp
   implicit none
   integer :: ncol, lm, lcldmh, lcldlm, u, k, n3
   integer :: sz(SWK_NIN), szo(SWK_NOUT)
   real(8) :: taucrit8
   real :: taucrit
   real(4), allocatable :: buf(:)
   real, allocatable :: a(:)
   type(c_ptr) :: fin(SWK_NIN), fout(SWK_NOUT)
   character(len=512) :: fi, fo
   call get_command_argument(1, fi); call get_command_argument(2, fo)
   open(newunit=u, file=trim(fi), access='stream', form='unformatted', status='old')
   read(u) ncol, lm, lcldmh, lcldlm
   read(u) taucrit8
   taucrit = real(taucrit8, kind(taucrit))
   n3 = ncol * lm
   sz = n3
   sz(SWK_PLE) = ncol * (lm + 1)
   sz(SWK_ZTH) = ncol
   do k = 1, SWK_NIN
      allocate(buf(sz(k)), a(sz(k))); read(u) buf; a = real(buf, kind(a))
      fin(k) = dev_alloc(sz(k)); call dev_put(fin(k), a, sz(k))
      deallocate(buf, a)
   end do
   close(u)
   szo = ncol
   szo(SWK_FCLD_X:SWK_TAUCLS) = n3
   do k = 1, SWK_NOUT
      fout(k) = dev_alloc(szo(k))
   end do
   call sw_update_clouds(ncol, lm, lcldmh, lcldlm, taucrit, fin, fout)
   call dev_sync()
   open(newunit=u, file=trim(fo), access='stream', form='unformatted', status='replace')
   do k = 1, SWK_NOUT
      allocate(a(szo(k))); call dev_get(a, fout(k), szo(k)); write(u) real(a, 8); deallocate(a)
   end do
   close(u)
   do k = 1, SWK_NIN
      call dev_free(fin(k))
   end do
   do k = 1, SWK_NOUT
      call dev_free(fout(k))
   end do
end program swclouds_driver

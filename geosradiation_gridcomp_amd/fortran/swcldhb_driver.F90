! swcldhb_driver.F90 -- the heartbeat McICA cloud fractions of UPDATE_EXPORT as a GEOS_SolarGridComp built with SOLAR_RADVAL would run
! them every model step with its fields on the device (GEOS_SolarGridComp.F90:7060-7223): set_inhomogeneity as RAD:Initialize calls it,
! FCLD, PLE, T, QI, QL, LATS in, `call sw_update_cldhb`, CLDTTSWHB / CLDHISWHB / CLDMDSWHB / CLDLOSWHB out.  Reads a batch written by
! tests/test_sw_cldhb.py (fields in SWHB_* order), writes the four exports in SWHB_* order as real(8).
program swcldhb_driver
   use iso_c_binding
   use cloud_condensate_inhomogeneity, only : set_inhomogeneity
   use geosrad_gridcomp
   implicit none
   integer :: ncol, lm, lcldmh, lcldlm, doy, ih, u, k
   integer :: sz(SWHB_NIN)
   real(4), allocatable :: buf(:)
   real, allocatable :: a(:)
   type(c_ptr) :: fin(SWHB_NIN), fout(SWHB_NOUT)
   character(len=512) :: fi, fo
   call get_command_argument(1, fi); call get_command_argument(2, fo)
   open(newunit=u, file=trim(fi), access='stream', form='unformatted', status='old')
   read(u) ncol, lm, lcldmh, lcldlm, doy, ih
   if (ih /= 0) call set_inhomogeneity(ih)
   sz = ncol * lm
   sz(SWHB_PLE) = ncol * (lm + 1)
   sz(SWHB_LATS) = ncol
   do k = 1, SWHB_NIN
      allocate(buf(sz(k)), a(sz(k))); read(u) buf; a = real(buf, kind(a))
      fin(k) = dev_alloc(sz(k)); call dev_put(fin(k), a, sz(k))
      deallocate(buf, a)
   end do
   close(u)
   do k = 1, SWHB_NOUT
      fout(k) = dev_alloc(ncol)
   end do
   call sw_update_cldhb(ncol, lm, lcldmh, lcldlm, doy, fin, fout)
   call dev_sync()
   open(newunit=u, file=trim(fo), access='stream', form='unformatted', status='replace')
   allocate(a(ncol))
   do k = 1, SWHB_NOUT
      call dev_get(a, fout(k), ncol); write(u) real(a, 8)
   end do
   close(u)
   do k = 1, SWHB_NIN
      call dev_free(fin(k))
   end do
   do k = 1, SWHB_NOUT
      call dev_free(fout(k))
   end do
end program swcldhb_driver

! swchou_na_driver.F90 -- the Chou-Suarez branch of SORADCORE with the aerosol-free internals from the same call: where
! GEOS_SolarGridComp runs SORADCORE a second time with include_aerosols = .false. when a *NA export is requested
! (GEOS_SolarGridComp.F90:3249-3259, internals :3997-4016), one `call sw_driver_chou_na` fills FSWN ... and FSWNAN, FSCNAN, FSWUNAN,
! FSCUNAN, FSWBANDNAN.  Reads a batch written by tests/test_fortran_sorad_na.py (fields in SWC_* order, as swchou_driver reads them),
! prints the sums of FSW and FSWNA at the surface and writes FSW, FSWBAND and the five aerosol-free internals.
program swchou_na_driver
   use iso_c_binding
   use geosrad_gridcomp
   implicit none
   integer :: ncol, lm, lcldmh, lcldlm, u, k, rc, n3, n3p
   integer :: sz(SWC_NIN), nsz(SWCNA_NOUT)
   real(8) :: consts(SWC_NCONST)
   real(4), allocatable :: buf(:)
   real(4) :: hk4(35)
   real :: hk_uv(5), hk_ir(3,10)
   real, allocatable :: a(:), fsw(:), fswband(:)
   type(c_ptr) :: fin(SWC_NIN), fout(SWC_NOUT), nout(SWCNA_NOUT)
   character(len=512) :: fi, fo
   call get_command_argument(1, fi); call get_command_argument(2, fo)
   open(newunit=u, file=trim(fi), access='stream', form='unformatted', status='old')
   read(u) ncol, lm, lcldmh, lcldlm
   read(u) consts
   n3 = ncol * lm; n3p = ncol * (lm + 1)
   sz = n3
   sz(SWC_PLE) = n3p
   sz([SWC_TAUA, SWC_SSAA, SWC_ASYA]) = n3 * 8
   sz([SWC_ZT, SWC_ALBVR, SWC_ALBVF, SWC_ALBNR, SWC_ALBNF]) = ncol
   do k = 1, SWC_NIN
      allocate(buf(sz(k)), a(sz(k))); read(u) buf; a = real(buf, kind(a))
      fin(k) = dev_alloc(sz(k)); call dev_put(fin(k), a, sz(k))
      deallocate(buf, a)
   end do
   read(u) hk4
   close(u)
   hk_uv = real(hk4(1:5), kind(hk_uv)); hk_ir = reshape(real(hk4(6:35), kind(hk_ir)), [3,10])
   do k = SWC_FSW, SWC_FSCU
      fout(k) = dev_alloc(n3p)
   end do
   do k = SWC_NIRR, SWC_UVRF
      fout(k) = dev_alloc(ncol)
   end do
   do k = SWC_FSWBAND, SWC_DFBAND
      fout(k) = dev_alloc(ncol * 8)
   end do
   nsz = n3p; nsz(SWCNA_FSWBANDNA) = ncol * 8
   do k = 1, SWCNA_NOUT
      nout(k) = dev_alloc(nsz(k))
   end do
   call sw_driver_chou_na(ncol, lm, fin, consts, lcldmh, lcldlm, hk_uv, hk_ir, .true., fout, nout, rc)
   if (rc /= 0) error stop 'sw_driver_chou_na failed'
   call dev_sync()
   allocate(fsw(n3p), fswband(ncol * 8))
   call dev_get(fsw, fout(SWC_FSW), n3p); call dev_get(fswband, fout(SWC_FSWBAND), ncol * 8)
   open(newunit=u, file=trim(fo), access='stream', form='unformatted', status='replace')
   write(u) real(fsw,8), real(fswband,8)
   print '(a,es24.16)', 'FSW(sfc) ', sum(real(fsw(n3p - ncol + 1:n3p),8))
   do k = 1, SWCNA_NOUT
      allocate(a(nsz(k)))
      call dev_get(a, nout(k), nsz(k))
      write(u) real(a,8)
      if (k == SWCNA_FSWNA) print '(a,es24.16)', 'FSWNA(sfc) ', sum(real(a(n3p - ncol + 1:n3p),8))
      deallocate(a)
   end do
   close(u)
   do k = 1, SWC_NIN
      call dev_free(fin(k))
   end do
   do k = 1, SWC_NOUT
      call dev_free(fout(k))
   end do
   do k = 1, SWCNA_NOUT
      call dev_free(nout(k))
   end do
end program swchou_na_driver

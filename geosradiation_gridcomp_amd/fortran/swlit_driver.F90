! swlit_driver.F90 -- the Chou-Suarez branch of SORADCORE as GEOS_SolarGridComp would run it with its UN-PACKED fields on the device
! (GEOS_SolarGridComp.F90:3686 `daytime = ZTH > 0.`, PackIt :3839-3894, SORADCORE :4484-4572, UnPackIt :6520-6580): `call lit_index` on ZTH,
! then one `call sw_driver_chou_lit` on the tile's fields; the dark columns of FSW .. FSWBAND receive their DEFAULT, those of DRBAND keep
! what they held.  Reads a batch written by tests/test_fortran_sw_lit.py (ZTH, then the fields in SWC_* order), writes NumLit and FSW, FSWU,
! NIRR, FSWBAND, DRBAND.
program swlit_driver
   use iso_c_binding
   use geosrad_gridcomp
   implicit none
   integer :: ncol, lm, lcldmh, lcldlm, u, k, rc, n3, n3p, NumLit
   integer :: sz(SWC_NIN)
   real(8) :: consts(SWC_NCONST)
   real(4), allocatable :: buf(:)
   real(4) :: hk4(35), dark4(SWC_NOUT), sentinel4
   real :: hk_uv(5), hk_ir(3,10), dark(SWC_NOUT)
   logical :: keep(SWC_NOUT)
   real, allocatable :: a(:), fsw(:), fswu(:), nirr(:), fswband(:), drband(:)
   type(c_ptr) :: fin(SWC_NIN), fout(SWC_NOUT), d_zth, d_idx, d_pos, d_nlit
   character(len=512) :: fi, fo
   call get_command_argument(1, fi); call get_command_argument(2, fo)
   open(newunit=u, file=trim(fi), access='stream', form='unformatted', status='old')
   read(u) ncol, lm, lcldmh, lcldlm
   read(u) consts
   allocate(buf(ncol), a(ncol)); read(u) buf; a = real(buf, kind(a))
   d_zth = dev_alloc(ncol); call dev_put(d_zth, a, ncol)
   deallocate(buf, a)
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
   read(u) dark4, sentinel4
   close(u)
   hk_uv = real(hk4(1:5), kind(hk_uv)); hk_ir = reshape(real(hk4(6:35), kind(hk_ir)), [3,10])
   dark = real(dark4, kind(dark))
   keep = .false.; keep(SWC_DRBAND) = .true.
   do k = SWC_FSW, SWC_FSCU
      fout(k) = dev_alloc(n3p)
   end do
   do k = SWC_NIRR, SWC_UVRF
      fout(k) = dev_alloc(ncol)
   end do
   do k = SWC_FSWBAND, SWC_DFBAND
      fout(k) = dev_alloc(ncol * 8)
   end do
   allocate(drband(ncol * 8))
   drband = real(sentinel4, kind(drband)); call dev_put(fout(SWC_DRBAND), drband, ncol * 8)
   ! the index arrays are default integers: an integer takes no more room than a real
   d_idx = dev_alloc(ncol); d_pos = dev_alloc(ncol); d_nlit = dev_alloc(1)
   call lit_index(ncol, d_zth, d_idx, d_pos, d_nlit, NumLit)
   call sw_driver_chou_lit(ncol, NumLit, d_idx, d_pos, lm, fin, consts, lcldmh, lcldlm, hk_uv, hk_ir, .true., dark, keep, fout, rc)
   if (rc /= 0) error stop 'sw_driver_chou_lit failed'
   call dev_sync()
   allocate(fsw(n3p), fswu(n3p), nirr(ncol), fswband(ncol * 8))
   call dev_get(fsw, fout(SWC_FSW), n3p); call dev_get(fswu, fout(SWC_FSWU), n3p); call dev_get(nirr, fout(SWC_NIRR), ncol)
   call dev_get(fswband, fout(SWC_FSWBAND), ncol * 8); call dev_get(drband, fout(SWC_DRBAND), ncol * 8)
   open(newunit=u, file=trim(fo), access='stream', form='unformatted', status='replace')
   write(u) real(NumLit,8), real(fsw,8), real(fswu,8), real(nirr,8), real(fswband,8), real(drband,8)
   close(u)
   do k = 1, SWC_NIN
      call dev_free(fin(k))
   end do
   do k = 1, SWC_NOUT
      call dev_free(fout(k))
   end do
   call dev_free(d_zth); call dev_free(d_idx); call dev_free(d_pos); call dev_free(d_nlit)
end program swlit_driver

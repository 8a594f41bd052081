! lwna_driver.F90 -- the RRTMG branch of LW_Driver with the aerosol-free INTERNALs the reference leaves undefined there
! (GEOS_IrradGridComp.F90:3552-3556), followed by one heartbeat Update_Flx that reads them as real fields (USE_RRTMG semantics off,
! :3861-3999): GEOS-native fields on the device in, the exports FLXA, FLA, OLRA, LWSA out.
! Reads a batch written by tests/test_fortran_lw_na.py (fields in LWD_* order), prints the sums of the exports of a step with
! TSINST = TS + 1 K and writes FLXA_INT, FLA_INT, DFDTSNA and the exports FLXA, FLA, OLRA, LWSA.
program lwna_driver
   use iso_c_binding
   use rrtmg_lw_init, only : rrtmg_lw_ini
   use cloud_condensate_inhomogeneity, only : set_inhomogeneity
   use geosrad_gridcomp
   implicit none
   integer :: ncol, lm, nb, doy, lcldlm, lcldmh, ih, u, k, n3, n3p
   integer :: sz(LWD_NIN)
   real(8) :: consts(LWD_NCONST)
   real(4), allocatable :: buf(:)
   real, allocatable :: a(:), ts(:), flxa_int(:), fla_int(:), dfdtsna(:), flxa(:), fla(:), olra(:), lwsa(:)
   type(c_ptr) :: fin(LWD_NIN), fout(LWD_NOUT), uin(LWU_NIN), uout(LWU_NOUT), d_tsinst, rout(LWD_NRATOUT), nout(LWNA_NOUT)
   character(len=6) :: nameRATS(1) = ['      ']
   logical :: bo(16)
   character(len=512) :: fi, fo
   call get_command_argument(1, fi); call get_command_argument(2, fo)
   open(newunit=u, file=trim(fi), access='stream', form='unformatted', status='old')
   read(u) ncol, lm, nb, ih, doy, lcldlm, lcldmh
   read(u) consts
   n3 = ncol * lm; n3p = ncol * (lm + 1)
   sz = n3
   sz(LWD_PLE) = n3p; sz(LWD_TAUA) = n3 * nb; sz(LWD_SSAA) = n3 * nb
   sz([LWD_TS, LWD_EMIS, LWD_LATS, LWD_T2M]) = ncol
   sz(LWD_CO2_3D) = 0
   fin = c_null_ptr
   allocate(ts(ncol))
   do k = 1, LWD_NIN
      if (sz(k) == 0) cycle
      allocate(buf(sz(k)), a(sz(k))); read(u) buf; a = real(buf, kind(a))
      fin(k) = dev_alloc(sz(k)); call dev_put(fin(k), a, sz(k))
      if (k == LWD_TS) ts = a
      deallocate(buf, a)
   end do
   close(u)
   fout = c_null_ptr
   do k = LWD_FLXU_INT, LWD_FLC_INT
      if (k == LWD_DFDTSNA .or. k == LWD_DFDTSCNA) cycle      ! the INTERNAL state takes the real ones, below
      fout(k) = dev_alloc(n3p)
   end do
   do k = LWD_SFCEM_INT, LWD_CLDLOLW
      fout(k) = dev_alloc(ncol)
   end do
   do k = 1, LWNA_NOUT
      nout(k) = dev_alloc(n3p)
   end do
   call set_inhomogeneity(ih)
   call rrtmg_lw_ini
   bo = .false.
   rout = c_null_ptr
   call lw_driver_rrtmg_na(ncol, lm, nb, fin, consts, 3, 1, doy, lcldlm, lcldmh, bo, fout, 0, nameRATS(1:0), rout, nout)
   ! heartbeat: the surface has warmed by 1 K since the full calculation
   d_tsinst = dev_alloc(ncol)
   ts = ts + 1.0
   call dev_put(d_tsinst, ts, ncol)
   uin = c_null_ptr; uout = c_null_ptr
   uin(LWU_TSINST) = d_tsinst; uin(LWU_TS_INT) = fout(LWD_TS_INT); uin(LWU_SFCEM_INT) = fout(LWD_SFCEM_INT); uin(LWU_FCLD) = fin(LWD_FCLD)
   uin(LWU_FLX_INT) = fout(LWD_FLX_INT); uin(LWU_FLC_INT) = fout(LWD_FLC_INT); uin(LWU_FLXU_INT) = fout(LWD_FLXU_INT)
   uin(LWU_FLCU_INT) = fout(LWD_FLCU_INT); uin(LWU_FLXD_INT) = fout(LWD_FLXD_INT); uin(LWU_FLCD_INT) = fout(LWD_FLCD_INT)
   uin(LWU_DFDTS) = fout(LWD_DFDTS); uin(LWU_DFDTSC) = fout(LWD_DFDTSC)
   uin(LWU_FLXA_INT) = nout(LWNA_FLXA_INT); uin(LWU_FLA_INT) = nout(LWNA_FLA_INT); uin(LWU_FLXAU_INT) = nout(LWNA_FLXAU_INT)
   uin(LWU_FLAU_INT) = nout(LWNA_FLAU_INT); uin(LWU_FLXAD_INT) = nout(LWNA_FLXAD_INT); uin(LWU_FLAD_INT) = nout(LWNA_FLAD_INT)
   uin(LWU_DFDTSNA) = nout(LWNA_DFDTSNA); uin(LWU_DFDTSCNA) = nout(LWNA_DFDTSCNA)
   uout(LWU_FLXA) = dev_alloc(n3p); uout(LWU_FLA) = dev_alloc(n3p); uout(LWU_OLRA) = dev_alloc(ncol); uout(LWU_LWSA) = dev_alloc(ncol)
   call lw_update_flx(ncol, lm, .false., lcldmh, lcldlm, 1.0e15, uin, uout)
   call dev_sync()
   allocate(flxa_int(n3p), fla_int(n3p), dfdtsna(n3p), flxa(n3p), fla(n3p), olra(ncol), lwsa(ncol))
   call dev_get(flxa_int, nout(LWNA_FLXA_INT), n3p); call dev_get(fla_int, nout(LWNA_FLA_INT), n3p)
   call dev_get(dfdtsna, nout(LWNA_DFDTSNA), n3p)
   call dev_get(flxa, uout(LWU_FLXA), n3p); call dev_get(fla, uout(LWU_FLA), n3p); call dev_get(olra, uout(LWU_OLRA), ncol)
   call dev_get(lwsa, uout(LWU_LWSA), ncol)
   print '(a,3es24.16)', 'FLXA FLA OLRA ', sum(real(flxa,8)), sum(real(fla,8)), sum(real(olra,8))
   open(newunit=u, file=trim(fo), access='stream', form='unformatted', status='replace')
   write(u) real(flxa_int,8), real(fla_int,8), real(dfdtsna,8), real(flxa,8), real(fla,8), real(olra,8), real(lwsa,8)
   close(u)
   do k = 1, LWD_NIN
      call dev_free(fin(k))
   end do
   do k = 1, LWD_NOUT
      call dev_free(fout(k))
   end do
   do k = 1, LWNA_NOUT
      call dev_free(nout(k))
   end do
end program lwna_driver

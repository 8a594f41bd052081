! swobio_driver.F90 -- the SOLAR TO OBIO conversion of UPDATE_EXPORT as GEOS_SolarGridComp would run it with its fields on the device
! (GEOS_SolarGridComp.F90:7584-7737, USE_OCEANOBIOGEOCHEM: 1): one `call sw_update_obio` per model step turns SLR and the internals DRBANDN /
! DFBANDN (IM,JM,14) of the RRTMG branch into the exports DROBIO / DFOBIO (IM,JM,33); a second call with DFOBIO not associated shows the
! export left alone.  Reads a batch written by tests/test_fortran_sw_obio.py (SLR, DRBANDN, DFBANDN), writes DROBIO, DFOBIO and the DROBIO
! of the second call.
program swobio_driver
   use iso_c_binding
   use geosrad_gridcomp
   implicit none
   integer, parameter :: nbands = 14
   integer :: ncol, u
   real(4), allocatable :: buf(:)
   real, allocatable :: slr(:), xr(:), xf(:), drobio(:), dfobio(:), dr2(:)
   type(c_ptr) :: d_slr, d_dr, d_df, d_dro, d_dfo
   character(len=512) :: fi, fo
   call get_command_argument(1, fi); call get_command_argument(2, fo)
   open(newunit=u, file=trim(fi), access='stream', form='unformatted', status='old')
   read(u) ncol
   allocate(slr(ncol), xr(ncol * nbands), xf(ncol * nbands), drobio(ncol * NB_OBIO), dfobio(ncol * NB_OBIO), dr2(ncol * NB_OBIO))
   allocate(buf(ncol)); read(u) buf; slr = real(buf, kind(slr)); deallocate(buf)
   allocate(buf(ncol * nbands)); read(u) buf; xr = real(buf, kind(xr)); read(u) buf; xf = real(buf, kind(xf)); deallocate(buf)
   close(u)
   d_slr = dev_alloc(ncol); d_dr = dev_alloc(ncol * nbands); d_df = dev_alloc(ncol * nbands)
   d_dro = dev_alloc(ncol * NB_OBIO); d_dfo = dev_alloc(ncol * NB_OBIO)
   call dev_put(d_slr, slr, ncol); call dev_put(d_dr, xr, ncol * nbands); call dev_put(d_df, xf, ncol * nbands)
   call sw_update_obio(ncol, OBIO_RRTMG, nbands, d_slr, d_dr, d_df, d_dro, d_dfo)
   call dev_sync()
   call dev_get(drobio, d_dro, ncol * NB_OBIO); call dev_get(dfobio, d_dfo, ncol * NB_OBIO)
   ! DFOBIO not associated: DROBIO from the diffuse internal this time, DFOBIO keeps the first call's values
   call sw_update_obio(ncol, OBIO_RRTMG, nbands, d_slr, d_df, c_null_ptr, d_dro, c_null_ptr)
   call dev_sync()
   call dev_get(dr2, d_dro, ncol * NB_OBIO)
   open(newunit=u, file=trim(fo), access='stream', form='unformatted', status='replace')
   write(u) real(drobio,8), real(dfobio,8), real(dr2,8)
   close(u)
   call dev_free(d_slr); call dev_free(d_dr); call dev_free(d_df); call dev_free(d_dro); call dev_free(d_dfo)
end program swobio_driver

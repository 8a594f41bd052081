! sw_radval_driver.F90 -- sw_driver.F90's call of the solver as a GEOS build configured with ENABLE_SOLAR_RADVAL makes it
! (GEOS_SolarGridComp.F90:6331 with the SOLAR_RADVAL actual arguments): linked against the shim modules compiled -DSOLAR_RADVAL, the
! reference's long argument list (rrtmg_sw_rad.F90:68-124).  Reads a column batch written by tests/test_fortran_sw_radval.py (sw_driver's
! format plus iceflgsw) and writes the fluxes, the cot family and the 120 diagnostics back.
program sw_radval_driver
   use rrtmg_sw_init, only : rrtmg_sw_ini
   use rrtmg_sw_rad, only : rrtmg_sw
   use parrrsw, only : nbndsw
   use cloud_condensate_inhomogeneity, only : set_inhomogeneity
   implicit none
   integer :: ncol, nlay, ih, dyofyr, cloudLM, cloudMH, iaer, normFlx, isolvar, iceflg, u, i, rc, mapl_placeholder
   real(4) :: scon4
   real(4), allocatable :: buf(:)
   real, allocatable, dimension(:,:) :: play, plev, tlay, h2o, o3, co2, ch4, o2, cld, ciwp, clwp, rei, rel, zm, &
      swuflx, swdflx, swuflxc, swdflxc, fswband, rv
   real, pointer, dimension(:,:) :: drband, dfband
   real, allocatable, dimension(:) :: coszen, alat, asdir, asdif, aldir, aldif, nirr, nirf, parr, parf, uvrr, uvrf, &
      c1, c2, c3, c4, c5, c6, c7, c8
   real, allocatable, dimension(:,:,:) :: tauaer, ssaaer, asmaer
   integer, allocatable :: cc(:,:)
   character(len=512) :: fin, fout
   call get_command_argument(1, fin); call get_command_argument(2, fout)
   open(newunit=u, file=trim(fin), access='stream', form='unformatted', status='old')
   read(u) ncol, nlay, ih, dyofyr, cloudLM, cloudMH, iaer, normFlx, isolvar, scon4, iceflg
   allocate(play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay), h2o(ncol,nlay), o3(ncol,nlay), co2(ncol,nlay), ch4(ncol,nlay), &
      o2(ncol,nlay), cld(ncol,nlay), ciwp(ncol,nlay), clwp(ncol,nlay), rei(ncol,nlay), rel(ncol,nlay), zm(ncol,nlay), &
      coszen(ncol), alat(ncol), asdir(ncol), asdif(ncol), aldir(ncol), aldif(ncol), tauaer(ncol,nlay,nbndsw), &
      ssaaer(ncol,nlay,nbndsw), asmaer(ncol,nlay,nbndsw), cc(ncol,4), swuflx(ncol,nlay+1), swdflx(ncol,nlay+1), &
      swuflxc(ncol,nlay+1), swdflxc(ncol,nlay+1), nirr(ncol), nirf(ncol), parr(ncol), parf(ncol), uvrr(ncol), uvrf(ncol), &
      fswband(ncol,nbndsw), drband(ncol,nbndsw), dfband(ncol,nbndsw), c1(ncol), c2(ncol), c3(ncol), c4(ncol), c5(ncol), &
      c6(ncol), c7(ncol), c8(ncol), rv(ncol,120))
   call rd1(coszen); call rd2(play); call rd2(plev); call rd2(tlay); call rd2(h2o); call rd2(o3); call rd2(co2); call rd2(ch4)
   call rd2(o2); call rd2(cld); call rd2(ciwp); call rd2(clwp); call rd2(rei); call rd2(rel); call rd2(zm); call rd1(alat)
   do i = 1, nbndsw
      call rd2(tauaer(:,:,i))
   end do
   do i = 1, nbndsw
      call rd2(ssaaer(:,:,i))
   end do
   do i = 1, nbndsw
      call rd2(asmaer(:,:,i))
   end do
   call rd1(asdir); call rd1(asdif); call rd1(aldir); call rd1(aldif)
   close(u)
   if (ih /= 0) call set_inhomogeneity(ih)
   call rrtmg_sw_ini
   mapl_placeholder = 0
   rv = -1.
   ! the 120 SOLAR_RADVAL actual arguments in the reference's order: column k of rv is the k-th of cdsdtp .. forinlp
   call rrtmg_sw(mapl_placeholder, 4, ncol, nlay, real(scon4), 1.0, coszen, isolvar, play, plev, tlay, h2o, o3, co2, ch4, o2, &
      iceflg, 1, cld, ciwp, clwp, rei, rel, dyofyr, zm, alat, iaer, tauaer, ssaaer, asmaer, asdir, asdif, aldir, aldif, &
      cloudLM, cloudMH, normFlx, cc, swuflx, swdflx, swuflxc, swdflxc, nirr, nirf, parr, parf, uvrr, uvrf, fswband, &
      c1, c2, c3, c4, c5, c6, c7, c8, &
      rv(:,1), rv(:,2), rv(:,3), rv(:,4), &
      rv(:,5), rv(:,6), rv(:,7), rv(:,8), &
      rv(:,9), rv(:,10), rv(:,11), rv(:,12), &
      rv(:,13), rv(:,14), rv(:,15), rv(:,16), &
      rv(:,17), rv(:,18), rv(:,19), rv(:,20), &
      rv(:,21), rv(:,22), rv(:,23), rv(:,24), &
      rv(:,25), rv(:,26), rv(:,27), rv(:,28), &
      rv(:,29), rv(:,30), rv(:,31), rv(:,32), &
      rv(:,33), rv(:,34), rv(:,35), rv(:,36), &
      rv(:,37), rv(:,38), rv(:,39), rv(:,40), &
      rv(:,41), rv(:,42), rv(:,43), rv(:,44), &
      rv(:,45), rv(:,46), rv(:,47), rv(:,48), &
      rv(:,49), rv(:,50), rv(:,51), rv(:,52), &
      rv(:,53), rv(:,54), rv(:,55), rv(:,56), &
      rv(:,57), rv(:,58), rv(:,59), rv(:,60), &
      rv(:,61), rv(:,62), rv(:,63), rv(:,64), &
      rv(:,65), rv(:,66), rv(:,67), rv(:,68), &
      rv(:,69), rv(:,70), rv(:,71), rv(:,72), &
      rv(:,73), rv(:,74), rv(:,75), rv(:,76), &
      rv(:,77), rv(:,78), rv(:,79), rv(:,80), &
      rv(:,81), rv(:,82), rv(:,83), rv(:,84), &
      rv(:,85), rv(:,86), rv(:,87), rv(:,88), &
      rv(:,89), rv(:,90), rv(:,91), rv(:,92), &
      rv(:,93), rv(:,94), rv(:,95), rv(:,96), &
      rv(:,97), rv(:,98), rv(:,99), rv(:,100), &
      rv(:,101), rv(:,102), rv(:,103), rv(:,104), &
      rv(:,105), rv(:,106), rv(:,107), rv(:,108), &
      rv(:,109), rv(:,110), rv(:,111), rv(:,112), &
      rv(:,113), rv(:,114), rv(:,115), rv(:,116), &
      rv(:,117), rv(:,118), rv(:,119), rv(:,120), &
      .true., drband, dfband, RC=rc)
   open(newunit=u, file=trim(fout), access='stream', form='unformatted', status='replace')
   write(u) rc, real(swuflx,8), real(swdflx,8), real(swuflxc,8), real(swdflxc,8), real(nirr,8), real(parf,8), real(fswband,8), &
      real(drband,8), real(dfband,8), real(c1,8), real(c2,8), real(c3,8), real(c4,8), real(c5,8), real(c6,8), real(c7,8), real(c8,8), &
      real(rv,8), cc
   close(u)
contains
   subroutine rd2(a)
      real, intent(out) :: a(:,:)
      if (allocated(buf)) deallocate(buf)
      allocate(buf(size(a))); read(u) buf; a = reshape(real(buf, kind(a)), shape(a))
   end subroutine
   subroutine rd1(a)
      real, intent(out) :: a(:)
      if (allocated(buf)) deallocate(buf)
      allocate(buf(size(a))); read(u) buf; a = real(buf, kind(a))
   end subroutine
end program sw_radval_driver

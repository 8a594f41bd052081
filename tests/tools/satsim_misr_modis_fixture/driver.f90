! driver.f90 -- calls the reference's own `MISR_simulator` (compiled unmodified from GEOSsatsim_GridComp by make_fixture.py, never copied)
! on the batch make_fixture.py writes, and writes back what it leaves.  It holds no line of the reference: one call.
! in.bin: npoints, nlev, ncol; sunlit (integers); zfull, at, dtau_s, dtau_c (npoints,nlev), frac_out (npoints,ncol,nlev), missing_value,
! all default reals of this build.  out.bin: fq_MISR_TAU_v_CTH (npoints,7,16), dist_model_layertops (npoints,16), MISR_mean_ztop,
! MISR_cldarea (npoints).  The outputs are filled with -7 before the call, so that what the routine does not set is seen.
program driver
  implicit none
  integer :: npoints, nlev, ncol
  integer, allocatable :: sunlit(:)
  real, allocatable :: zfull(:,:), at(:,:), dtau_s(:,:), dtau_c(:,:), frac_out(:,:,:), fq(:,:,:), dist(:,:), ztop(:), area(:)
  real :: missing_value
  open(10, file='in.bin', access='stream', form='unformatted', status='old')
  read(10) npoints, nlev, ncol
  allocate(sunlit(npoints), zfull(npoints,nlev), at(npoints,nlev), dtau_s(npoints,nlev), dtau_c(npoints,nlev), frac_out(npoints,ncol,nlev))
  allocate(fq(npoints,7,16), dist(npoints,16), ztop(npoints), area(npoints))
  read(10) sunlit, zfull, at, dtau_s, dtau_c, frac_out, missing_value
  close(10)
  fq = -7.; dist = -7.; ztop = -7.; area = -7.
  call MISR_simulator(npoints, nlev, ncol, sunlit, zfull, at, dtau_s, dtau_c, frac_out, missing_value, fq, dist, ztop, area)
  open(11, file='out.bin', access='stream', form='unformatted', status='replace')
  write(11) fq, dist, ztop, area
  close(11)
end program

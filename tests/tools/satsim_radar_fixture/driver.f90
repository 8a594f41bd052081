! driver.f90 -- calls the reference's own `prec_scops` (llnl/prec_scops.f, compiled unmodified from GEOSsatsim_GridComp by make_fixture.py,
! never copied) on the arrays make_fixture.py writes, and writes back what it leaves.  It holds no line of the reference: one call.
! Built twice, in r4 and with -fdefault-real-8.
! in.bin: npoints, nlev, ncol; ls_p_rate, cv_p_rate (npoints,nlev); frac_out (npoints,ncol,nlev); all default reals of this build, the top
! of the atmosphere first (cosp.F90:404-411).  out.bin: prec_frac (npoints,ncol,nlev).
program driver
  implicit none
  integer :: npoints, nlev, ncol
  real, allocatable :: ls(:,:), cv(:,:), frac(:,:,:), prec(:,:,:)
  open(10, file='in.bin', access='stream', form='unformatted', status='old')
  read(10) npoints, nlev, ncol
  allocate(ls(npoints,nlev), cv(npoints,nlev), frac(npoints,ncol,nlev), prec(npoints,ncol,nlev))
  read(10) ls, cv, frac
  close(10)
  call prec_scops(npoints, nlev, ncol, ls, cv, frac, prec)
  open(11, file='out.bin', access='stream', form='unformatted', status='replace')
  write(11) prec
  close(11)
end program

! driver_modis.f90 -- calls the reference's own `modis_L2_simulator` (per point, as cosp_modis_simulator.F90:183-190 does) and
! `modis_L3_simulator` of module mod_modis_sim (compiled unmodified from GEOSsatsim_GridComp by make_fixture.py, never copied) on the
! per-sub-column arrays make_fixture.py writes, and writes back what they leave.  It holds no line of the reference: two calls.
! in_modis.bin: npoints (the sunlit ones), ncol, nlev; t, p (npoints,nlev), ph (npoints,nlev+1); tau, water, ice, rw, ri
! (npoints,ncol,nlev); isccp tau and cloud-top pressure (npoints,ncol); all default reals of this build.  out_modis.bin: phase
! (integers), ctp, tau, size (npoints,ncol); the 17 means in modis_L3_simulator's argument order (npoints each); the joint histogram
! (npoints,6,7).
program driver_modis
  use mod_modis_sim
  implicit none
  integer :: npoints, ncol, nlev, i
  real, allocatable :: t(:,:), p(:,:), ph(:,:), tau(:,:,:), water(:,:,:), ice(:,:,:), rw(:,:,:), ri(:,:,:), itau(:,:), ictp(:,:)
  integer, allocatable :: phase(:,:)
  real, allocatable :: ctp(:,:), rtau(:,:), rsize(:,:), m(:,:), hist(:,:,:)
  open(10, file='in_modis.bin', access='stream', form='unformatted', status='old')
  read(10) npoints, ncol, nlev
  allocate(t(npoints,nlev), p(npoints,nlev), ph(npoints,nlev+1), tau(npoints,ncol,nlev), water(npoints,ncol,nlev), ice(npoints,ncol,nlev))
  allocate(rw(npoints,ncol,nlev), ri(npoints,ncol,nlev), itau(npoints,ncol), ictp(npoints,ncol))
  allocate(phase(npoints,ncol), ctp(npoints,ncol), rtau(npoints,ncol), rsize(npoints,ncol), m(npoints,17), hist(npoints,6,7))
  read(10) t, p, ph, tau, water, ice, rw, ri, itau, ictp
  close(10)
  do i = 1, npoints
     call modis_L2_simulator(t(i,:), p(i,:), ph(i,:), tau(i,:,:), water(i,:,:), ice(i,:,:), rw(i,:,:), ri(i,:,:), itau(i,:), ictp(i,:), &
                             phase(i,:), ctp(i,:), rtau(i,:), rsize(i,:))
  end do
  call modis_L3_simulator(phase, ctp, rtau, rsize, m(:,1), m(:,2), m(:,3), m(:,4), m(:,5), m(:,6), m(:,7), m(:,8), m(:,9), m(:,10), m(:,11), &
                          m(:,12), m(:,13), m(:,14), m(:,15), m(:,16), m(:,17), hist)
  open(11, file='out_modis.bin', access='stream', form='unformatted', status='replace')
  write(11) phase, ctp, rtau, rsize, m, hist
  close(11)
end program

! driver.f90 -- calls the reference's own `lidar_simulator` once per sub-column (as cosp_lidar.F90:63-80 does) and `diag_lidar` of module
! mod_lmd_ipsl_stats on the collected arrays (as cosp_stats.F90:126-130 does), both compiled unmodified from GEOSsatsim_GridComp by
! make_fixture.py, never copied, on the arrays make_fixture.py writes, and writes back what they leave.  It holds no line of the reference:
! two calls.  Everything is in the reference's own level order, the surface first; make_fixture.py does the flips.
! in.bin: npoints, nlev, ncol, ice_type; p, t (npoints,nlev); presf (npoints,nlev+1); the four in-cloud contents (npoints,ncol,nlev); the
! four gridbox radii (npoints,nlev); frac_out (npoints,ncol,nlev); land (npoints); pplay (npoints,nlev); all default reals of this build.
! out.bin: pmol (npoints,nlev); pnorm, tautot (npoints,ncol,nlev); refl (npoints,ncol,5); lidarcld (npoints,nlev); cldlayer (npoints,4);
! cfad_sr (npoints,15,nlev); parasolrefl (npoints,5); srbval (15).
program driver
  use mod_cosp_constants, only: LIDAR_UNDEF, SR_BINS, PARASOL_NREFL, LIDAR_NCAT
  use mod_lmd_ipsl_stats
  implicit none
  integer :: npoints, nlev, ncol, ice_type, i
  real, allocatable :: p(:,:), t(:,:), presf(:,:), mr(:,:,:,:), reff(:,:,:), frac(:,:,:), land(:), pplay(:,:)
  real, allocatable :: pmol(:,:), pnorm(:,:,:), tautot(:,:,:), refl(:,:,:), b1(:,:), t1(:,:), r1(:,:), f1(:,:), q(:,:,:)
  real, allocatable :: lidarcld(:,:), cldlayer(:,:), cfad(:,:,:), parasolrefl(:,:), srbval(:)
  open(10, file='in.bin', access='stream', form='unformatted', status='old')
  read(10) npoints, nlev, ncol, ice_type
  allocate(p(npoints,nlev), t(npoints,nlev), presf(npoints,nlev+1), mr(npoints,ncol,nlev,4), reff(npoints,nlev,4), frac(npoints,ncol,nlev))
  allocate(land(npoints), pplay(npoints,nlev))
  allocate(pmol(npoints,nlev), pnorm(npoints,ncol,nlev), tautot(npoints,ncol,nlev), refl(npoints,ncol,PARASOL_NREFL))
  allocate(b1(npoints,nlev), t1(npoints,nlev), r1(npoints,PARASOL_NREFL), f1(npoints,nlev), q(npoints,nlev,4))
  allocate(lidarcld(npoints,nlev), cldlayer(npoints,LIDAR_NCAT), cfad(npoints,SR_BINS,nlev), parasolrefl(npoints,PARASOL_NREFL), srbval(SR_BINS))
  read(10) p, t, presf, mr, reff, frac, land, pplay
  close(10)
  do i = 1, ncol
     q = mr(:,i,:,:)
     f1 = frac(:,i,:)
     call lidar_simulator(npoints, nlev, 4, PARASOL_NREFL, LIDAR_UNDEF, p, presf, t, q(:,:,1), q(:,:,2), q(:,:,3), q(:,:,4), &
                          reff(:,:,1), reff(:,:,2), reff(:,:,3), reff(:,:,4), f1, ice_type, pmol, b1, t1, r1)
     pnorm(:,i,:) = b1
     tautot(:,i,:) = t1
     refl(:,i,:) = r1
  end do
  call diag_lidar(npoints, ncol, nlev, SR_BINS, PARASOL_NREFL, pnorm, pmol, refl, land, pplay, LIDAR_UNDEF, .true., cfad, srbval, &
                  LIDAR_NCAT, lidarcld, cldlayer, parasolrefl)
  open(11, file='out.bin', access='stream', form='unformatted', status='replace')
  write(11) pmol, pnorm, tautot, refl, lidarcld, cldlayer, cfad, parasolrefl, srbval
  close(11)
end program

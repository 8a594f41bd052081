! driver.f90 -- calls the reference's own `scops` and `icarus` (compiled unmodified from GEOSsatsim_GridComp by make_fixture.py, never
! copied) on the batch make_fixture.py writes, and writes back what they leave.  It holds no line of the reference: two calls.
! in.bin: npoints, nlev, ncol; sunlit, seed (integers); pfull, phalf (nlev + 1), qv, cc, conv, dtau_s, dtau_c, at, dem_s, dem_c
! (npoints,nlev), skt (npoints), emsfc_lw, all default reals of this build.  out.bin: for overlap 1, 2, 3 frac_out and the seeds; then for
! top_height 1, 2, 3 x top_height_direction 1, 2 on the overlap = 3 mask every output of icarus in its argument order.
! With a number N as the argument: N timed calls of scops + icarus (overlap 3, top_height 1, direction 2), nothing written.
program driver
  implicit none
  integer :: npoints, nlev, ncol, ov, th, thd, rep, nrep
  integer, allocatable :: sunlit(:), seed0(:), seed(:)
  real, allocatable :: pfull(:,:), phalf(:,:), qv(:,:), cc(:,:), conv(:,:), dtau_s(:,:), dtau_c(:,:), at(:,:), dem_s(:,:), dem_c(:,:), skt(:)
  real, allocatable :: frac_out(:,:,:), fq(:,:,:), tca(:), mpt(:), mtau(:), malb(:), mtb(:), mtbc(:), boxtau(:,:), boxptop(:,:)
  real :: emsfc_lw
  integer(8) :: c0, c1, cr
  character(len=32) :: arg
  nrep = 0
  if (command_argument_count() >= 1) then
     call get_command_argument(1, arg); read(arg, *) nrep
  end if
  open(10, file='in.bin', access='stream', form='unformatted', status='old')
  read(10) npoints, nlev, ncol
  allocate(sunlit(npoints), seed0(npoints), seed(npoints), pfull(npoints,nlev), phalf(npoints,nlev+1), qv(npoints,nlev), cc(npoints,nlev))
  allocate(conv(npoints,nlev), dtau_s(npoints,nlev), dtau_c(npoints,nlev), at(npoints,nlev), dem_s(npoints,nlev), dem_c(npoints,nlev), skt(npoints))
  allocate(frac_out(npoints,ncol,nlev), fq(npoints,7,7), tca(npoints), mpt(npoints), mtau(npoints), malb(npoints), mtb(npoints), mtbc(npoints))
  allocate(boxtau(npoints,ncol), boxptop(npoints,ncol))
  read(10) sunlit, seed0, pfull, phalf, qv, cc, conv, dtau_s, dtau_c, at, dem_s, dem_c, skt, emsfc_lw
  close(10)
  if (nrep > 0) then
     call system_clock(c0, cr)
     do rep = 1, nrep
        seed = seed0
        call scops(npoints, nlev, ncol, seed, cc, conv, 3, frac_out, 0)
        call icarus(0, 0, npoints, sunlit, nlev, ncol, pfull, phalf, qv, cc, conv, dtau_s, dtau_c, 1, 2, 3, frac_out, skt, emsfc_lw, at, &
                    dem_s, dem_c, fq, tca, mpt, mtau, malb, mtb, mtbc, boxtau, boxptop)
     end do
     call system_clock(c1)
     print '(a,i0,a,i0,a,f10.3,a)', 'scops+icarus, ', npoints, ' points x ', nrep, ' calls: ', 1.0d3*dble(c1-c0)/dble(cr)/nrep, ' ms per call'
     stop
  end if
  open(11, file='out.bin', access='stream', form='unformatted', status='replace')
  do ov = 1, 3
     seed = seed0
     call scops(npoints, nlev, ncol, seed, cc, conv, ov, frac_out, 0)
     write(11) frac_out, seed
  end do
  do th = 1, 3
     do thd = 1, 2
        call icarus(0, 0, npoints, sunlit, nlev, ncol, pfull, phalf, qv, cc, conv, dtau_s, dtau_c, th, thd, 3, frac_out, skt, emsfc_lw, at, &
                    dem_s, dem_c, fq, tca, mpt, mtau, malb, mtb, mtbc, boxtau, boxptop)
        write(11) fq, tca, mpt, mtau, malb, mtb, mtbc, boxtau, boxptop
     end do
  end do
  close(11)
end program

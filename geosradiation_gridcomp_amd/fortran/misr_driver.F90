! misr_driver.F90 -- a caller of the drop-in externals `scops` (satsim_shims.F90) and `MISR_simulator` (misr_modis_shims.F90) in the way COSP
! calls the reference's (cosp.F90:397, cosp_misr_simulator.F90:72-74): no interface block, explicit-shape arrays from the top of the
! atmosphere down, the mask handed from one to the other as the real array it is in Fortran.
! Reads npoints, nlev, ncol, overlap, then sunlit, seed (integers) and cc, conv, zfull, at, dtau_s, dtau_c (npoints,nlev) and missing_value as
! real(4), written by tests/test_fortran_misr.py; writes every result as real(8) in the order of the `write` statements below.
program misr_driver
   implicit none
   integer :: npoints, nlev, ncol, overlap, u, k
   integer, allocatable :: sunlit(:), seed(:)
   real(4), allocatable :: b2(:,:)
   real(4) :: m4
   real, allocatable :: a(:,:,:), frac_out(:,:,:), fq(:,:,:), dist(:,:), ztop(:), area(:)
   real, allocatable :: p(:,:), ph(:,:), zero(:,:), rl(:,:), boxptop(:,:), mmean(:,:), mhist(:,:,:)
   real :: missing_value
   character(len=512) :: fi, fo
   ! a(:,:,k): 1 cc, 2 conv, 3 zfull, 4 at, 5 dtau_s, 6 dtau_c
   call get_command_argument(1, fi); call get_command_argument(2, fo)
   open(newunit=u, file=trim(fi), access='stream', form='unformatted', status='old')
   read(u) npoints, nlev, ncol, overlap
   allocate(sunlit(npoints), seed(npoints), b2(npoints,nlev), a(npoints,nlev,6))
   read(u) sunlit, seed
   do k = 1, 6
      read(u) b2; a(:,:,k) = b2
   end do
   read(u) m4; missing_value = m4
   close(u)
   allocate(frac_out(npoints,ncol,nlev), fq(npoints,7,16), dist(npoints,16), ztop(npoints), area(npoints))
   open(newunit=u, file=trim(fo), access='stream', form='unformatted', status='replace')

   call scops(npoints,nlev,ncol,seed,a(:,:,1),a(:,:,2),overlap,frac_out,0)
   write(u) real(frac_out, 8)

   call MISR_simulator(npoints,nlev,ncol,sunlit,a(:,:,3),a(:,:,4),a(:,:,5),a(:,:,6),frac_out,missing_value,fq,dist,ztop,area)
   write(u) real(fq, 8), real(dist, 8), real(ztop, 8), real(area, 8)

   ! the batched MODIS call on the same mask: t = at, p and ph from zfull (any positive, increasing pressures do for a caller's demo), the
   ! stratiform water content dtau_s / 1000 as liquid with a 10 micron radius, no ice, no convection, ISCCP's cloud top at 800 hPa
   allocate(p(npoints,nlev), ph(npoints,nlev+1), zero(npoints,nlev), rl(npoints,nlev), boxptop(npoints,ncol), mmean(npoints,17), mhist(npoints,7,7))
   p = 101325. * exp(-a(:,:,3) / 7400.); ph(:,1) = 0.; ph(:,2:nlev) = 0.5 * (p(:,1:nlev-1) + p(:,2:nlev)); ph(:,nlev+1) = 101325.
   zero = 0.; rl = 1.0e-5; boxptop = 800.
   call geosrad_modis_simulator(npoints,nlev,ncol,sunlit,a(:,:,4),p,ph,a(:,:,5),a(:,:,6),frac_out,a(:,:,5)/1000.,zero,zero,zero,rl,zero,zero,zero, &
                                boxptop,mmean,mhist)
   write(u) real(mmean, 8), real(mhist, 8)
   close(u)
end program misr_driver

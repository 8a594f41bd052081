! lidar_driver.F90 -- a caller of the drop-in external `scops` (satsim_shims.F90) and of the batched `geosrad_lidar_simulator`
! (lidar_shims.F90): no interface block, explicit-shape arrays from the top of the atmosphere down, the mask handed from one to the other as
! the real array it is in Fortran.
! Reads npoints, nlev, ncol, overlap, ice_type, then seed (integers) and cc, conv, p, t, pplay, the four contents and the four radii
! (npoints,nlev), presf (npoints,nlev+1) and land (npoints) as real(4), written by tests/test_fortran_lidar.py; writes every result as real(8)
! in the order of the `write` statements below.
program lidar_driver
   implicit none
   integer :: npoints, nlev, ncol, overlap, ice_type, u, k
   integer, allocatable :: seed(:)
   real(4), allocatable :: b2(:,:), b3(:,:), b1(:)
   real, allocatable :: a(:,:,:), presf(:,:), land(:), frac_out(:,:,:), lidarcld(:,:), cldlayer(:,:), cfad(:,:,:), parasol(:,:), pmol(:,:)
   character(len=512) :: fi, fo
   ! a(:,:,k): 1 cc, 2 conv, 3 p, 4 t, 5 pplay, 6-9 mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, 10-13 reff_lsliq, reff_lsice, reff_cvliq, reff_cvice
   call get_command_argument(1, fi); call get_command_argument(2, fo)
   open(newunit=u, file=trim(fi), access='stream', form='unformatted', status='old')
   read(u) npoints, nlev, ncol, overlap, ice_type
   allocate(seed(npoints), b2(npoints,nlev), b3(npoints,nlev+1), b1(npoints), a(npoints,nlev,13), presf(npoints,nlev+1), land(npoints))
   read(u) seed
   do k = 1, 13
      read(u) b2; a(:,:,k) = b2
   end do
   read(u) b3; presf = b3
   read(u) b1; land = b1
   close(u)
   allocate(frac_out(npoints,ncol,nlev), lidarcld(npoints,nlev), cldlayer(npoints,4), cfad(npoints,15,nlev), parasol(npoints,5), pmol(npoints,nlev))
   open(newunit=u, file=trim(fo), access='stream', form='unformatted', status='replace')

   call scops(npoints,nlev,ncol,seed,a(:,:,1),a(:,:,2),overlap,frac_out,0)
   write(u) real(frac_out, 8)

   call geosrad_lidar_simulator(npoints,nlev,ncol,ice_type,a(:,:,3),a(:,:,4),presf,a(:,:,5),frac_out,a(:,:,6),a(:,:,7),a(:,:,8),a(:,:,9), &
                                a(:,:,10),a(:,:,11),a(:,:,12),a(:,:,13),land,lidarcld,cldlayer,cfad,parasol,pmol)
   write(u) real(lidarcld, 8), real(cldlayer, 8), real(cfad, 8), real(parasol, 8), real(pmol, 8)
   close(u)
end program lidar_driver

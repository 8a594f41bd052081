! satsim_driver.F90 -- a caller of the drop-in externals `scops` and `icarus` of satsim_shims.F90 in the way COSP calls the reference's
! (cosp.F90:397, cosp_isccp_simulator.F90:74-80): no interface block, explicit-shape arrays from the top of the atmosphere down, literal
! zeros for the debug arguments, the mask handed from one to the other as the real array it is in Fortran.
! Reads npoints, nlev, ncol, overlap, top_height, top_height_direction, then sunlit, seed (integers) and pfull, phalf (nlev + 1), qv, cc,
! conv, dtau_s, dtau_c, at, dem_s, dem_c (npoints,nlev), skt (npoints) and emsfc_lw as real(4), written by tests/test_fortran_satsim.py;
! writes the seeds as integers and every result as real(8) in the order of the `write` statements below.
program satsim_driver
   implicit none
   integer :: npoints, nlev, ncol, overlap, top_height, top_height_direction, u, k
   integer, allocatable :: sunlit(:), seed(:)
   real(4), allocatable :: b1(:), b2(:,:), b3(:,:)
   real(4) :: e4
   real, allocatable :: a(:,:,:), phalf(:,:), skt(:), frac_out(:,:,:)
   real, allocatable :: fq_isccp(:,:,:), totalcldarea(:), meanptop(:), meantaucld(:), meanalbedocld(:), meantb(:), meantbclr(:), boxtau(:,:), boxptop(:,:)
   real :: emsfc_lw
   character(len=512) :: fi, fo
   ! a(:,:,k): 1 pfull, 2 qv, 3 cc, 4 conv, 5 dtau_s, 6 dtau_c, 7 at, 8 dem_s, 9 dem_c
   call get_command_argument(1, fi); call get_command_argument(2, fo)
   open(newunit=u, file=trim(fi), access='stream', form='unformatted', status='old')
   read(u) npoints, nlev, ncol, overlap, top_height, top_height_direction
   allocate(sunlit(npoints), seed(npoints), b1(npoints), b2(npoints,nlev), b3(npoints,nlev+1), skt(npoints), a(npoints,nlev,9), phalf(npoints,nlev+1))
   read(u) sunlit, seed
   read(u) b2; a(:,:,1) = b2
   read(u) b3; phalf = b3
   do k = 2, 9
      read(u) b2; a(:,:,k) = b2
   end do
   read(u) b1; skt = b1
   read(u) e4; emsfc_lw = e4
   close(u)
   allocate(frac_out(npoints,ncol,nlev), fq_isccp(npoints,7,7), totalcldarea(npoints), meanptop(npoints), meantaucld(npoints))
   allocate(meanalbedocld(npoints), meantb(npoints), meantbclr(npoints), boxtau(npoints,ncol), boxptop(npoints,ncol))
   open(newunit=u, file=trim(fo), access='stream', form='unformatted', status='replace')

   call scops(npoints,nlev,ncol,seed,a(:,:,3),a(:,:,4),overlap,frac_out,0)
   write(u) seed
   write(u) real(frac_out, 8)

   call icarus(0,0,npoints,sunlit,nlev,ncol,a(:,:,1),phalf,a(:,:,2),a(:,:,3),a(:,:,4),a(:,:,5),a(:,:,6),top_height,top_height_direction,overlap, &
               frac_out,skt,emsfc_lw,a(:,:,7),a(:,:,8),a(:,:,9),fq_isccp,totalcldarea,meanptop,meantaucld,meanalbedocld,meantb,meantbclr,boxtau,boxptop)
   write(u) real(fq_isccp, 8), real(totalcldarea, 8), real(meanptop, 8), real(meantaucld, 8), real(meanalbedocld, 8), real(meantb, 8), &
            real(meantbclr, 8), real(boxtau, 8), real(boxptop, 8)
   close(u)
end program satsim_driver

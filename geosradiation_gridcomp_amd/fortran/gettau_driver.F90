! gettau_driver.F90 -- the callers of GEOS_RadiationShared/gettau.F90 against the drop-in module gettau (gettau_shims.F90), in their own
! argument shapes:
!   - the Solar GridComp's `use gettau, only: getvistau` (GEOS_SolarGridComp.F90:177) and its call per column on strided sections of
!     (IM,JM,LM[,4]) arrays with ict = LCLDMH, icb = LCLDLM (:7264-7272);
!   - the satellite simulator's `use gettau` and its calls with ict = icb = 0: getvistau and getirtau band 4 (GEOS_SatsimGridComp.F90:3427-3432);
!   - one batched call of each routine on the same fields as (IM*JM,LM[,4]) arrays: the form to use.
! Reads IM, JM, LM, LCLDMH, LCLDLM and ZTH (IM,JM), DP, CLIN (IM,JM,LM), REFF, HYDROMETS (IM,JM,LM,4) as real(4), written by
! tests/test_fortran_gettau.py; writes every result as real(8) in the order of the `write` statements below.
module solar_caller
   use gettau, only: getvistau                     ! GEOS_SolarGridComp.F90:177
   implicit none
contains
   subroutine update_export_tau(IM, JM, LM, LCLDMH, LCLDLM, ZTH, DP, CLIN, REFF, HYDROMETS, TAUBEAM, TAUCLD, ASY)
      integer, intent(in) :: IM, JM, LM, LCLDMH, LCLDLM
      real, intent(in) :: ZTH(IM,JM), DP(IM,JM,LM), CLIN(IM,JM,LM), REFF(IM,JM,LM,4), HYDROMETS(IM,JM,LM,4)
      real, intent(out) :: TAUBEAM(IM,JM,LM,4), TAUCLD(IM,JM,LM,4), ASY(IM,JM,LM)
      integer :: I, J
      DO I = 1,IM
         DO J = 1,JM
            CALL GETVISTAU( &
               LM,ZTH(I,J),DP(I,J,:),&
               CLIN(I,J,:),REFF(I,J,:,:),HYDROMETS(I,J,:,:),&
               LCLDMH,LCLDLM,&
               TAUBEAM(I,J,:,:),TAUCLD(I,J,:,:),ASY(I,J,:))
         END DO
      END DO
   end subroutine
end module solar_caller

module satsim_caller
   use gettau                                      ! GEOS_SatsimGridComp.F90
   implicit none
contains
   subroutine satsim_tau(im, jm, lm, mcosz, delp, FCLD, reff, cwc, tausw, taulw, tcl, en)
      integer, intent(in) :: im, jm, lm
      real, intent(in) :: mcosz(im,jm), delp(im,jm,lm), FCLD(im,jm,lm), reff(im,jm,lm,4), cwc(im,jm,lm,4)
      real, intent(out) :: tausw(im,jm,lm,4), taulw(im,jm,lm,4), tcl(im,jm,0:lm), en(im,jm,0:lm)
      real :: dumtaubeam(lm,4), dumasycl(lm), dumtcldlyr(0:lm), dumenn(0:lm)
      integer :: i, j
      do i = 1, im
         do j = 1, jm
            call getvistau(lm,mcosz(i,j),delp(i,j,:),FCLD(i,j,:),reff(i,j,:,:),cwc(i,j,:,:),0,0,&
                           dumtaubeam(:,:),tausw(i,j,:,:),dumasycl(:))
            call getirtau(4,lm,delp(i,j,:),FCLD(i,j,:),reff(i,j,:,:),cwc(i,j,:,:),&
                          taulw(i,j,:,:),dumtcldlyr(:),dumenn(:))
            tcl(i,j,:) = dumtcldlyr; en(i,j,:) = dumenn
         end do
      end do
   end subroutine
end module satsim_caller

program gettau_driver
   use gettau
   use solar_caller
   use satsim_caller
   implicit none
   integer :: IM, JM, LM, LCLDMH, LCLDLM, u, n
   real(4), allocatable :: b2(:,:), b3(:,:,:), b4(:,:,:,:)
   real, allocatable :: ZTH(:,:), DP(:,:,:), CLIN(:,:,:), REFF(:,:,:,:), HYD(:,:,:,:)
   real, allocatable :: TB(:,:,:,:), TD(:,:,:,:), ASY(:,:,:), TSW(:,:,:,:), TLW(:,:,:,:), TCL(:,:,:), EN(:,:,:)
   real, allocatable :: c1(:), d2(:,:), f2(:,:), r3(:,:,:), h3(:,:,:), o3a(:,:,:), o3b(:,:,:), o2a(:,:), o2b(:,:), l2a(:,:), l2b(:,:)
   character(len=512) :: fi, fo
   call get_command_argument(1, fi); call get_command_argument(2, fo)
   open(newunit=u, file=trim(fi), access='stream', form='unformatted', status='old')
   read(u) IM, JM, LM, LCLDMH, LCLDLM
   allocate(b2(IM,JM), b3(IM,JM,LM), b4(IM,JM,LM,4))
   allocate(ZTH(IM,JM), DP(IM,JM,LM), CLIN(IM,JM,LM), REFF(IM,JM,LM,4), HYD(IM,JM,LM,4))
   read(u) b2; ZTH = real(b2, kind(ZTH))
   read(u) b3; DP = real(b3, kind(DP))
   read(u) b3; CLIN = real(b3, kind(CLIN))
   read(u) b4; REFF = real(b4, kind(REFF))
   read(u) b4; HYD = real(b4, kind(HYD))
   close(u)
   n = IM * JM
   allocate(TB(IM,JM,LM,4), TD(IM,JM,LM,4), ASY(IM,JM,LM), TSW(IM,JM,LM,4), TLW(IM,JM,LM,4), TCL(IM,JM,0:LM), EN(IM,JM,0:LM))
   open(newunit=u, file=trim(fo), access='stream', form='unformatted', status='replace')

   call update_export_tau(IM, JM, LM, LCLDMH, LCLDLM, ZTH, DP, CLIN, REFF, HYD, TB, TD, ASY)
   write(u) real(TB, 8), real(TD, 8), real(ASY, 8)
   call satsim_tau(IM, JM, LM, ZTH, DP, CLIN, REFF, HYD, TSW, TLW, TCL, EN)
   write(u) real(TSW, 8), real(TLW, 8), real(TCL, 8), real(EN, 8)

   ! batched: the same fields as (IM*JM, LM[, 4]) arrays, one call each
   allocate(c1(n), d2(n,LM), f2(n,LM), r3(n,LM,4), h3(n,LM,4), o3a(n,LM,4), o3b(n,LM,4), o2a(n,LM), o2b(n,LM), l2a(n,0:LM), l2b(n,0:LM))
   c1 = reshape(ZTH, [n]); d2 = reshape(DP, [n,LM]); f2 = reshape(CLIN, [n,LM]); r3 = reshape(REFF, [n,LM,4]); h3 = reshape(HYD, [n,LM,4])
   call getvistau(LM, c1, d2, f2, r3, h3, LCLDMH, LCLDLM, o3a, o3b, o2a)
   write(u) real(o3a, 8), real(o3b, 8), real(o2a, 8)
   call getnirtau(2, LM, c1, d2, f2, r3, h3, LCLDMH, LCLDLM, o3a, o3b, o2a, o2b)
   write(u) real(o3a, 8), real(o3b, 8), real(o2a, 8), real(o2b, 8)
   call getirtau(3, LM, d2, f2, r3, h3, o3a, l2a, l2b)
   write(u) real(o3a, 8), real(l2a, 8), real(l2b, 8)
   close(u)
end program gettau_driver

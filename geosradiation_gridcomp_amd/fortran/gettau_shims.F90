! gettau_shims.F90 -- drop-in module with the REFERENCE's module and procedure names for GEOS_RadiationShared/gettau.F90; the bodies call
! the C ABI of include/geosrad_gettau.h.  Callers: `use gettau, only: getvistau` (GEOS_SolarGridComp.F90:177, call at :7266-7270),
! `use gettau` (GEOS_SatsimGridComp.F90, calls at :3427-3432), irrad.F90:645, sorad.F90:421-436, :955-968.
!   gettau : getvistau   gettau.F90:33-34
!            getnirtau   gettau.F90:102-103
!            getirtau    gettau.F90:173-174
! Each name is a generic with two specifics:
!   - the reference's own per-column signature (dp(:), reff(:,:) as (nlevs,4), scalar cosz).  It accepts the strided sections the
!     reference's callers pass (delp(i,j,:), reff(i,j,:,:)), copies them to contiguous temporaries and runs a one-column batch: one
!     column (1,nlevs,4) has the memory order of (nlevs,4).  Every call is a round trip over PCIe - a drop-in, not a fast path.
!   - the batched one: cosz(:), dp(:,:), reff(:,:,:) with the column index first, ncol = size(dp,1) columns in one call.  This is the
!     one to use: the loops over (I,J) around the reference's calls become one call on (IM*JM, LM[, 4]) arrays.
! MAPL_GRAV: MAPL_ConstantsMod's under -DGEOSRAD_WITH_MAPL, else the value the library's sorad and irrad kernels carry.
! The Chou-Suarez coefficient tables (module data of rad_constants in the reference) are uploaded on the first call that needs them.
module gettau
   use iso_c_binding
   use geosrad_c, only: geosrad_ctx_handle, geosrad_fail, geosrad_data_path, geosrad_load_tables_chou_lw, geosrad_load_tables_chou_sw
#ifdef GEOSRAD_WITH_MAPL
   use MAPL_ConstantsMod, only: MAPL_GRAV
#endif
   implicit none
   private
   public :: getvistau, getnirtau, getirtau

#ifndef GEOSRAD_WITH_MAPL
   real, parameter :: MAPL_GRAV = 9.80665
#endif
   logical, save :: loaded_sw = .false., loaded_lw = .false.

   interface getvistau
      module procedure getvistau_column, getvistau_batch
   end interface
   interface getnirtau
      module procedure getnirtau_column, getnirtau_batch
   end interface
   interface getirtau
      module procedure getirtau_column, getirtau_batch
   end interface

   interface
      integer(c_int) function geosrad_getvistau(ctx, ncol, nlevs, cosz, dp, fcld, reff, hydromets, ict, icb, grav, taubeam, taudiff, asycl) &
            bind(C, name='geosrad_getvistau')
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: ctx, cosz, dp, fcld, reff, hydromets, taubeam, taudiff, asycl
         integer(c_int), value :: ncol, nlevs, ict, icb
         real(c_double), value :: grav
      end function
      integer(c_int) function geosrad_getnirtau(ctx, ib, ncol, nlevs, cosz, dp, fcld, reff, hydromets, ict, icb, grav, taubeam, taudiff, &
            asycl, ssacl) bind(C, name='geosrad_getnirtau')
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: ctx, cosz, dp, fcld, reff, hydromets, taubeam, taudiff, asycl, ssacl
         integer(c_int), value :: ib, ncol, nlevs, ict, icb
         real(c_double), value :: grav
      end function
      integer(c_int) function geosrad_getirtau(ctx, ib, ncol, nlevs, dp, fcld, reff, hydromets, grav, taudiag, tcldlyr, enn) &
            bind(C, name='geosrad_getirtau')
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: ctx, dp, fcld, reff, hydromets, taudiag, tcldlyr, enn
         integer(c_int), value :: ib, ncol, nlevs
         real(c_double), value :: grav
      end function
   end interface

contains

   subroutine need_tables(lw)
      logical, intent(in) :: lw
      integer(c_int) :: rc
      real :: x
      if (lw) then
         if (loaded_lw) return
         rc = geosrad_load_tables_chou_lw(geosrad_ctx_handle(), geosrad_data_path(merge('chou_lw_r4.grtb', 'chou_lw_r8.grtb', kind(x) == 4)))
         loaded_lw = .true.
      else
         if (loaded_sw) return
         rc = geosrad_load_tables_chou_sw(geosrad_ctx_handle(), geosrad_data_path(merge('chou_sw_r4.grtb', 'chou_sw_r8.grtb', kind(x) == 4)))
         loaded_sw = .true.
      end if
      if (rc /= 0) call geosrad_fail('gettau (tables)')
   end subroutine

   ! ---- batched: ncol = size(dp,1) columns ------------------------------------------------------------------------------------
   subroutine getvistau_batch(nlevs,cosz,dp,fcld,reff,hydromets,ict,icb,taubeam,taudiff,asycl)
      integer, intent(IN ) :: nlevs
      real,    intent(IN ), target, contiguous :: cosz(:), dp(:,:), fcld(:,:), reff(:,:,:), hydromets(:,:,:)
      integer, intent(IN ) :: ict, icb
      real,    intent(OUT), target, contiguous :: taubeam(:,:,:), taudiff(:,:,:), asycl(:,:)
      integer(c_int) :: rc
      call need_tables(.false.)
      rc = geosrad_getvistau(geosrad_ctx_handle(), int(size(dp,1),c_int), int(nlevs,c_int), c_loc(cosz), c_loc(dp), c_loc(fcld), c_loc(reff), &
         c_loc(hydromets), int(ict,c_int), int(icb,c_int), real(MAPL_GRAV,c_double), c_loc(taubeam), c_loc(taudiff), c_loc(asycl))
      if (rc /= 0) call geosrad_fail('getvistau')
   end subroutine

   subroutine getnirtau_batch(ib,nlevs,cosz,dp,fcld,reff,hydromets,ict,icb,taubeam,taudiff,asycl,ssacl)
      integer, intent(IN ) :: ib, nlevs
      real,    intent(IN ), target, contiguous :: cosz(:), dp(:,:), fcld(:,:), reff(:,:,:), hydromets(:,:,:)
      integer, intent(IN ) :: ict, icb
      real,    intent(OUT), target, contiguous :: taubeam(:,:,:), taudiff(:,:,:), asycl(:,:), ssacl(:,:)
      integer(c_int) :: rc
      call need_tables(.false.)
      rc = geosrad_getnirtau(geosrad_ctx_handle(), int(ib,c_int), int(size(dp,1),c_int), int(nlevs,c_int), c_loc(cosz), c_loc(dp), c_loc(fcld), &
         c_loc(reff), c_loc(hydromets), int(ict,c_int), int(icb,c_int), real(MAPL_GRAV,c_double), c_loc(taubeam), c_loc(taudiff), &
         c_loc(asycl), c_loc(ssacl))
      if (rc /= 0) call geosrad_fail('getnirtau')
   end subroutine

   subroutine getirtau_batch(ib,nlevs,dp,fcld,reff,hydromets,taudiag,tcldlyr,enn)
      integer, intent(IN ) :: ib, nlevs
      real,    intent(IN ), target, contiguous :: dp(:,:), fcld(:,:), reff(:,:,:), hydromets(:,:,:)
      real,    intent(OUT), target, contiguous :: taudiag(:,:,:)
      real,    intent(OUT), target, contiguous :: tcldlyr(:,0:), enn(:,0:)
      integer(c_int) :: rc
      call need_tables(.true.)
      rc = geosrad_getirtau(geosrad_ctx_handle(), int(ib,c_int), int(size(dp,1),c_int), int(nlevs,c_int), c_loc(dp), c_loc(fcld), c_loc(reff), &
         c_loc(hydromets), real(MAPL_GRAV,c_double), c_loc(taudiag), c_loc(tcldlyr), c_loc(enn))
      if (rc /= 0) call geosrad_fail('getirtau')
   end subroutine

   ! ---- the reference's per-column signatures: contiguous copies, a batch of one column ------------------------------------------
   subroutine getvistau_column(nlevs,cosz,dp,fcld,reff,hydromets,ict,icb,taubeam,taudiff,asycl)
      integer, intent(IN ) :: nlevs
      real,    intent(IN ) :: cosz
      real,    intent(IN ) :: dp(:), fcld(:), reff(:,:), hydromets(:,:)
      integer, intent(IN ) :: ict, icb
      real,    intent(OUT) :: taubeam(:,:), taudiff(:,:), asycl(:)
      real :: c1(1), d(1,nlevs), f(1,nlevs), r(1,nlevs,4), h(1,nlevs,4), tb(1,nlevs,4), td(1,nlevs,4), as(1,nlevs)
      c1(1) = cosz; d(1,:) = dp(1:nlevs); f(1,:) = fcld(1:nlevs); r(1,:,:) = reff(1:nlevs,1:4); h(1,:,:) = hydromets(1:nlevs,1:4)
      call getvistau_batch(nlevs,c1,d,f,r,h,ict,icb,tb,td,as)
      taubeam(1:nlevs,1:4) = tb(1,:,:); taudiff(1:nlevs,1:4) = td(1,:,:); asycl(1:nlevs) = as(1,:)
   end subroutine

   subroutine getnirtau_column(ib,nlevs,cosz,dp,fcld,reff,hydromets,ict,icb,taubeam,taudiff,asycl,ssacl)
      integer, intent(IN ) :: ib, nlevs
      real,    intent(IN ) :: cosz
      real,    intent(IN ) :: dp(:), fcld(:), reff(:,:), hydromets(:,:)
      integer, intent(IN ) :: ict, icb
      real,    intent(OUT) :: taubeam(:,:), taudiff(:,:), asycl(:), ssacl(:)
      real :: c1(1), d(1,nlevs), f(1,nlevs), r(1,nlevs,4), h(1,nlevs,4), tb(1,nlevs,4), td(1,nlevs,4), as(1,nlevs), ss(1,nlevs)
      c1(1) = cosz; d(1,:) = dp(1:nlevs); f(1,:) = fcld(1:nlevs); r(1,:,:) = reff(1:nlevs,1:4); h(1,:,:) = hydromets(1:nlevs,1:4)
      call getnirtau_batch(ib,nlevs,c1,d,f,r,h,ict,icb,tb,td,as,ss)
      taubeam(1:nlevs,1:4) = tb(1,:,:); taudiff(1:nlevs,1:4) = td(1,:,:); asycl(1:nlevs) = as(1,:); ssacl(1:nlevs) = ss(1,:)
   end subroutine

   subroutine getirtau_column(ib,nlevs,dp,fcld,reff,hydromets,taudiag,tcldlyr,enn)
      integer, intent(IN ) :: ib, nlevs
      real,    intent(IN ) :: dp(:), fcld(:), reff(:,:), hydromets(:,:)
      real,    intent(OUT) :: taudiag(:,:)
      real,    intent(OUT) :: tcldlyr(0:), enn(0:)
      real :: d(1,nlevs), f(1,nlevs), r(1,nlevs,4), h(1,nlevs,4), tg(1,nlevs,4), tc(1,0:nlevs), en(1,0:nlevs)
      d(1,:) = dp(1:nlevs); f(1,:) = fcld(1:nlevs); r(1,:,:) = reff(1:nlevs,1:4); h(1,:,:) = hydromets(1:nlevs,1:4)
      call getirtau_batch(ib,nlevs,d,f,r,h,tg,tc,en)
      taudiag(1:nlevs,1:4) = tg(1,:,:); tcldlyr(0:nlevs) = tc(1,:); enn(0:nlevs) = en(1,:)
   end subroutine
end module gettau

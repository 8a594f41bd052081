! rrtmg_sw_shims.F90 -- drop-in modules with the REFERENCE's module and procedure names for the shortwave path;
! bodies call the C ABI.  GEOS_SolarGridComp.F90 `use`s exactly these names (GEOS_SolarGridComp.F90:179-181,
! 6678-6679), so linking this file instead of the reference's rrtmg_sw sources switches the SW hot path to the
! MI355X without touching the driver.
!
!   parrrsw          : nbndsw, ngptsw, jpband, jpb1, jpb2       (SW/modules/parrrsw.F90)
!   rrsw_wvn         : wavenum1, wavenum2                       (SW/modules/rrsw_wvn.F90, set in rrtmg_sw_init.F90:187-190)
!   rrtmg_sw_init    : rrtmg_sw_ini                             (SW/src/rrtmg_sw_init.F90:23)
!   rrtmg_sw_rad     : rrtmg_sw                                 (SW/src/rrtmg_sw_rad.F90:68-124)
!                      compiled with -DSOLAR_RADVAL, as a GEOS build configured with ENABLE_SOLAR_RADVAL compiles the reference
!                      (GEOSsolar_GridComp/CMakeLists.txt:18-21): the reference's long argument list (:86-119) over
!                      geosrad_rrtmg_sw_radval; without the flag nothing of it reaches the compiler
!
! The reference's rrtmg_sw takes the GridComp's MAPL handle only to drive timers; inside GEOS build this file with
! -DGEOSRAD_WITH_MAPL so the dummy has the reference's type, elsewhere it is an unlimited polymorphic placeholder.
module parrrsw
   implicit none
   integer, parameter :: nbndsw = 14, ngptsw = 112, jpband = 29, jpb1 = 16, jpb2 = 29, mxlay = 203
end module parrrsw

module rrsw_wvn
   use parrrsw, only : jpb1, jpb2
   implicit none
   real, parameter :: wavenum1(jpb1:jpb2) = [2600., 3250., 4000., 4650., 5150., 6150., 7700., 8050., 12850., 16000., 22650., &
                                             29000., 38000., 820.]
   real, parameter :: wavenum2(jpb1:jpb2) = [3250., 4000., 4650., 5150., 6150., 7700., 8050., 12850., 16000., 22650., 29000., &
                                             38000., 50000., 2600.]
   real, parameter :: delwave(jpb1:jpb2) = wavenum2 - wavenum1
end module rrsw_wvn

module rrtmg_sw_init
   use iso_c_binding
   use geosrad_c
   implicit none
   logical, save, private :: loaded = .false.
contains
   ! tables are uploaded to HBM once; later calls (GEOS_SolarGridComp.F90:6225 calls it every SW refresh) are no-ops
   subroutine rrtmg_sw_ini
      integer(c_int) :: rc
      real :: x
      if (loaded) return
      if (kind(x) == 4) then
         rc = geosrad_load_tables_sw(geosrad_ctx_handle(), geosrad_data_path('rrtmg_sw_r4.grtb'))
      else
         rc = geosrad_load_tables_sw(geosrad_ctx_handle(), geosrad_data_path('rrtmg_sw_r8.grtb'))
      end if
      if (rc /= 0) call geosrad_fail('rrtmg_sw_ini')
      loaded = .true.
   end subroutine rrtmg_sw_ini
end module rrtmg_sw_init

module rrtmg_sw_rad
   use iso_c_binding
   use geosrad_c
#ifdef GEOSRAD_WITH_MAPL
   use MAPL, only : MAPL_MetaComp, MAPL_TimerOn, MAPL_TimerOff
#endif
   implicit none
contains
   subroutine rrtmg_sw (MAPL, &
      rpart, ncol, nlay, &
      scon, adjes, coszen, isolvar, &
      play, plev, tlay, &
      h2ovmr, o3vmr, co2vmr, ch4vmr, o2vmr, &
      iceflgsw, liqflgsw, &
      cld, ciwp, clwp, rei, rel, &
      dyofyr, zm, alat, &
      iaer, tauaer, ssaaer, asmaer, &
      asdir, asdif, aldir, aldif, &
      cloudLM, cloudMH, normFlx, &
      clearCounts, swuflx, swdflx, swuflxc, swdflxc, &
      nirr, nirf, parr, parf, uvrr, uvrf, fswband, &
      cotdtp, cotdhp, cotdmp, cotdlp, &
      cotntp, cotnhp, cotnmp, cotnlp, &
#ifdef SOLAR_RADVAL
      cdsdtp, cdsdhp, cdsdmp, cdsdlp, &
      cdsntp, cdsnhp, cdsnmp, cdsnlp, &
      cotldtp, cotldhp, cotldmp, cotldlp, &
      cotlntp, cotlnhp, cotlnmp, cotlnlp, &
      cdsldtp, cdsldhp, cdsldmp, cdsldlp, &
      cdslntp, cdslnhp, cdslnmp, cdslnlp, &
      cotidtp, cotidhp, cotidmp, cotidlp, &
      cotintp, cotinhp, cotinmp, cotinlp, &
      cdsidtp, cdsidhp, cdsidmp, cdsidlp, &
      cdsintp, cdsinhp, cdsinmp, cdsinlp, &
      ssaldtp, ssaldhp, ssaldmp, ssaldlp, &
      ssalntp, ssalnhp, ssalnmp, ssalnlp, &
      sdsldtp, sdsldhp, sdsldmp, sdsldlp, &
      sdslntp, sdslnhp, sdslnmp, sdslnlp, &
      ssaidtp, ssaidhp, ssaidmp, ssaidlp, &
      ssaintp, ssainhp, ssainmp, ssainlp, &
      sdsidtp, sdsidhp, sdsidmp, sdsidlp, &
      sdsintp, sdsinhp, sdsinmp, sdsinlp, &
      asmldtp, asmldhp, asmldmp, asmldlp, &
      asmlntp, asmlnhp, asmlnmp, asmlnlp, &
      adsldtp, adsldhp, adsldmp, adsldlp, &
      adslntp, adslnhp, adslnmp, adslnlp, &
      asmidtp, asmidhp, asmidmp, asmidlp, &
      asmintp, asminhp, asminmp, asminlp, &
      adsidtp, adsidhp, adsidmp, adsidlp, &
      adsintp, adsinhp, adsinmp, adsinlp, &
      forldtp, forldhp, forldmp, forldlp, &
      forlntp, forlnhp, forlnmp, forlnlp, &
      foridtp, foridhp, foridmp, foridlp, &
      forintp, forinhp, forinmp, forinlp, &
#endif
      do_drfband, drband, dfband, &
      bndscl, indsolvar, solcycfrac, &
      RC)
      use parrrsw, only : nbndsw
#ifdef GEOSRAD_WITH_MAPL
      type(MAPL_MetaComp), pointer, intent(inout) :: MAPL
#else
      class(*), intent(inout) :: MAPL
#endif
      integer, intent(in) :: rpart, ncol, nlay
      real, intent(in) :: scon, adjes
      real, intent(in), target :: coszen(ncol)
      integer, intent(in) :: isolvar
      real, intent(in), target :: play(ncol,nlay), plev(ncol,nlay+1), tlay(ncol,nlay)
      real, intent(in), target, dimension(ncol,nlay) :: h2ovmr, o3vmr, co2vmr, ch4vmr, o2vmr, cld, ciwp, clwp, rei, rel, zm
      integer, intent(in) :: iceflgsw, liqflgsw, dyofyr, iaer, cloudLM, cloudMH, normFlx
      real, intent(in), target :: alat(ncol)
      real, intent(in), target, dimension(ncol,nlay,nbndsw) :: tauaer, ssaaer, asmaer
      real, intent(in), target, dimension(ncol) :: asdir, asdif, aldir, aldif
      integer, intent(out), target :: clearCounts(ncol,4)
      real, intent(out), target, dimension(ncol,nlay+1) :: swuflx, swdflx, swuflxc, swdflxc
      real, intent(out), target, dimension(ncol) :: nirr, nirf, parr, parf, uvrr, uvrf
      real, intent(out), target :: fswband(ncol,nbndsw)
      real, intent(out), target, dimension(ncol) :: cotdtp, cotdhp, cotdmp, cotdlp, cotntp, cotnhp, cotnmp, cotnlp
#ifdef SOLAR_RADVAL
      ! the cloud-optics validation diagnostics of the reference's SOLAR_RADVAL build (rrtmg_sw_rad.F90:86-119, declared :300 on)
      real, intent(out), dimension(ncol) :: cdsdtp, cdsdhp, cdsdmp, cdsdlp, cdsntp, cdsnhp, cdsnmp, cdsnlp
      real, intent(out), dimension(ncol) :: cotldtp, cotldhp, cotldmp, cotldlp, cotlntp, cotlnhp, cotlnmp, cotlnlp
      real, intent(out), dimension(ncol) :: cdsldtp, cdsldhp, cdsldmp, cdsldlp, cdslntp, cdslnhp, cdslnmp, cdslnlp
      real, intent(out), dimension(ncol) :: cotidtp, cotidhp, cotidmp, cotidlp, cotintp, cotinhp, cotinmp, cotinlp
      real, intent(out), dimension(ncol) :: cdsidtp, cdsidhp, cdsidmp, cdsidlp, cdsintp, cdsinhp, cdsinmp, cdsinlp
      real, intent(out), dimension(ncol) :: ssaldtp, ssaldhp, ssaldmp, ssaldlp, ssalntp, ssalnhp, ssalnmp, ssalnlp
      real, intent(out), dimension(ncol) :: sdsldtp, sdsldhp, sdsldmp, sdsldlp, sdslntp, sdslnhp, sdslnmp, sdslnlp
      real, intent(out), dimension(ncol) :: ssaidtp, ssaidhp, ssaidmp, ssaidlp, ssaintp, ssainhp, ssainmp, ssainlp
      real, intent(out), dimension(ncol) :: sdsidtp, sdsidhp, sdsidmp, sdsidlp, sdsintp, sdsinhp, sdsinmp, sdsinlp
      real, intent(out), dimension(ncol) :: asmldtp, asmldhp, asmldmp, asmldlp, asmlntp, asmlnhp, asmlnmp, asmlnlp
      real, intent(out), dimension(ncol) :: adsldtp, adsldhp, adsldmp, adsldlp, adslntp, adslnhp, adslnmp, adslnlp
      real, intent(out), dimension(ncol) :: asmidtp, asmidhp, asmidmp, asmidlp, asmintp, asminhp, asminmp, asminlp
      real, intent(out), dimension(ncol) :: adsidtp, adsidhp, adsidmp, adsidlp, adsintp, adsinhp, adsinmp, adsinlp
      real, intent(out), dimension(ncol) :: forldtp, forldhp, forldmp, forldlp, forlntp, forlnhp, forlnmp, forlnlp
      real, intent(out), dimension(ncol) :: foridtp, foridhp, foridmp, foridlp, forintp, forinhp, forinmp, forinlp
#endif
      logical, intent(in) :: do_drfband
      ! exactly the reference's dummies (rrtmg_sw_rad.F90:355): GEOS passes DRBAND / DFBAND disassociated unless SOLAR_TO_OBIO is
      ! set, and then as the non-contiguous section ptr2(1:Num2do,:) (GEOS_SolarGridComp.F90:778,4148-4151,6385)
      real, intent(inout), dimension(:,:), pointer :: drband, dfband
      real, intent(in), optional, target :: bndscl(nbndsw), indsolvar(2)
      real, intent(in), optional, target :: solcycfrac
      integer, intent(out), optional :: RC
      integer(c_int), target :: cc(ncol,4)
      integer(c_int) :: st
      type(c_ptr) :: pb, pi, pdr, pdf, pf
      real, allocatable, target :: zdr(:,:), zdf(:,:)       ! contiguous (ncol,nbndsw) images of the pointer targets
#ifdef SOLAR_RADVAL
      real, allocatable, target :: zrv(:,:)                 ! (ncol,120): the diagnostics in argument order, scattered below
      allocate(zrv(ncol,120))
#endif
      pb = c_null_ptr; pi = c_null_ptr; pdr = c_null_ptr; pdf = c_null_ptr; pf = c_null_ptr
      if (do_drfband) then                                   ! the pointers are touched only in this case, like the reference
         allocate(zdr(ncol,nbndsw), zdf(ncol,nbndsw))
         pdr = c_loc(zdr); pdf = c_loc(zdf)
      end if
      if (present(bndscl)) pb = c_loc(bndscl)
      if (present(indsolvar)) pi = c_loc(indsolvar)
      if (present(solcycfrac)) pf = c_loc(solcycfrac)        ! isolvar = 1 (rrtmg_sw_rad.F90:906-930)
      ! The reference's timers (rrtmg_sw_rad.F90:1181-1200 registers ---RRTMG_PART, _CLDSGEN, _CLDPRMC, _SETCOEF, _TAUMOL, _REFTRA, _VRTQDR):
      ! the whole call is one asynchronous pipeline here, so on the host it is charged to ---RRTMG_PART (the timer that brackets the
      ! reference's partition loop); the stages carry the reference's names as roctx ranges on the GPU timeline (GEOSRAD_ROCTX=1,
      ! rocprofv3 --marker-trace)
#ifdef GEOSRAD_WITH_MAPL
      call MAPL_TimerOn(MAPL, "---RRTMG_PART")
#endif
#ifdef SOLAR_RADVAL
      st = geosrad_rrtmg_sw_radval(geosrad_ctx_handle(), int(rpart,c_int), int(ncol,c_int), int(nlay,c_int), real(scon,c_double), &
         real(adjes,c_double), c_loc(coszen), int(isolvar,c_int), c_loc(play), c_loc(plev), c_loc(tlay), &
         c_loc(h2ovmr), c_loc(o3vmr), c_loc(co2vmr), c_loc(ch4vmr), c_loc(o2vmr), int(iceflgsw,c_int), int(liqflgsw,c_int), &
         c_loc(cld), c_loc(ciwp), c_loc(clwp), c_loc(rei), c_loc(rel), int(dyofyr,c_int), c_loc(zm), c_loc(alat), &
         int(iaer,c_int), c_loc(tauaer), c_loc(ssaaer), c_loc(asmaer), c_loc(asdir), c_loc(asdif), c_loc(aldir), c_loc(aldif), &
         int(cloudLM,c_int), int(cloudMH,c_int), int(normFlx,c_int), c_loc(cc), &
         c_loc(swuflx), c_loc(swdflx), c_loc(swuflxc), c_loc(swdflxc), &
         c_loc(nirr), c_loc(nirf), c_loc(parr), c_loc(parf), c_loc(uvrr), c_loc(uvrf), c_loc(fswband), &
         c_loc(cotdtp), c_loc(cotdhp), c_loc(cotdmp), c_loc(cotdlp), c_loc(cotntp), c_loc(cotnhp), c_loc(cotnmp), c_loc(cotnlp), &
         merge(1_c_int, 0_c_int, do_drfband), pdr, pdf, pb, pi, pf, c_loc(zrv))
#else
      st = geosrad_rrtmg_sw(geosrad_ctx_handle(), int(rpart,c_int), int(ncol,c_int), int(nlay,c_int), real(scon,c_double), &
         real(adjes,c_double), c_loc(coszen), int(isolvar,c_int), c_loc(play), c_loc(plev), c_loc(tlay), &
         c_loc(h2ovmr), c_loc(o3vmr), c_loc(co2vmr), c_loc(ch4vmr), c_loc(o2vmr), int(iceflgsw,c_int), int(liqflgsw,c_int), &
         c_loc(cld), c_loc(ciwp), c_loc(clwp), c_loc(rei), c_loc(rel), int(dyofyr,c_int), c_loc(zm), c_loc(alat), &
         int(iaer,c_int), c_loc(tauaer), c_loc(ssaaer), c_loc(asmaer), c_loc(asdir), c_loc(asdif), c_loc(aldir), c_loc(aldif), &
         int(cloudLM,c_int), int(cloudMH,c_int), int(normFlx,c_int), c_loc(cc), &
         c_loc(swuflx), c_loc(swdflx), c_loc(swuflxc), c_loc(swdflxc), &
         c_loc(nirr), c_loc(nirf), c_loc(parr), c_loc(parf), c_loc(uvrr), c_loc(uvrf), c_loc(fswband), &
         c_loc(cotdtp), c_loc(cotdhp), c_loc(cotdmp), c_loc(cotdlp), c_loc(cotntp), c_loc(cotnhp), c_loc(cotnmp), c_loc(cotnlp), &
         merge(1_c_int, 0_c_int, do_drfband), pdr, pdf, pb, pi, pf)
#endif
#ifdef GEOSRAD_WITH_MAPL
      call MAPL_TimerOff(MAPL, "---RRTMG_PART")
#endif
      clearCounts = cc
#ifdef SOLAR_RADVAL
      cdsdtp = zrv(:,1); cdsdhp = zrv(:,2); cdsdmp = zrv(:,3); cdsdlp = zrv(:,4)
      cdsntp = zrv(:,5); cdsnhp = zrv(:,6); cdsnmp = zrv(:,7); cdsnlp = zrv(:,8)
      cotldtp = zrv(:,9); cotldhp = zrv(:,10); cotldmp = zrv(:,11); cotldlp = zrv(:,12)
      cotlntp = zrv(:,13); cotlnhp = zrv(:,14); cotlnmp = zrv(:,15); cotlnlp = zrv(:,16)
      cdsldtp = zrv(:,17); cdsldhp = zrv(:,18); cdsldmp = zrv(:,19); cdsldlp = zrv(:,20)
      cdslntp = zrv(:,21); cdslnhp = zrv(:,22); cdslnmp = zrv(:,23); cdslnlp = zrv(:,24)
      cotidtp = zrv(:,25); cotidhp = zrv(:,26); cotidmp = zrv(:,27); cotidlp = zrv(:,28)
      cotintp = zrv(:,29); cotinhp = zrv(:,30); cotinmp = zrv(:,31); cotinlp = zrv(:,32)
      cdsidtp = zrv(:,33); cdsidhp = zrv(:,34); cdsidmp = zrv(:,35); cdsidlp = zrv(:,36)
      cdsintp = zrv(:,37); cdsinhp = zrv(:,38); cdsinmp = zrv(:,39); cdsinlp = zrv(:,40)
      ssaldtp = zrv(:,41); ssaldhp = zrv(:,42); ssaldmp = zrv(:,43); ssaldlp = zrv(:,44)
      ssalntp = zrv(:,45); ssalnhp = zrv(:,46); ssalnmp = zrv(:,47); ssalnlp = zrv(:,48)
      sdsldtp = zrv(:,49); sdsldhp = zrv(:,50); sdsldmp = zrv(:,51); sdsldlp = zrv(:,52)
      sdslntp = zrv(:,53); sdslnhp = zrv(:,54); sdslnmp = zrv(:,55); sdslnlp = zrv(:,56)
      ssaidtp = zrv(:,57); ssaidhp = zrv(:,58); ssaidmp = zrv(:,59); ssaidlp = zrv(:,60)
      ssaintp = zrv(:,61); ssainhp = zrv(:,62); ssainmp = zrv(:,63); ssainlp = zrv(:,64)
      sdsidtp = zrv(:,65); sdsidhp = zrv(:,66); sdsidmp = zrv(:,67); sdsidlp = zrv(:,68)
      sdsintp = zrv(:,69); sdsinhp = zrv(:,70); sdsinmp = zrv(:,71); sdsinlp = zrv(:,72)
      asmldtp = zrv(:,73); asmldhp = zrv(:,74); asmldmp = zrv(:,75); asmldlp = zrv(:,76)
      asmlntp = zrv(:,77); asmlnhp = zrv(:,78); asmlnmp = zrv(:,79); asmlnlp = zrv(:,80)
      adsldtp = zrv(:,81); adsldhp = zrv(:,82); adsldmp = zrv(:,83); adsldlp = zrv(:,84)
      adslntp = zrv(:,85); adslnhp = zrv(:,86); adslnmp = zrv(:,87); adslnlp = zrv(:,88)
      asmidtp = zrv(:,89); asmidhp = zrv(:,90); asmidmp = zrv(:,91); asmidlp = zrv(:,92)
      asmintp = zrv(:,93); asminhp = zrv(:,94); asminmp = zrv(:,95); asminlp = zrv(:,96)
      adsidtp = zrv(:,97); adsidhp = zrv(:,98); adsidmp = zrv(:,99); adsidlp = zrv(:,100)
      adsintp = zrv(:,101); adsinhp = zrv(:,102); adsinmp = zrv(:,103); adsinlp = zrv(:,104)
      forldtp = zrv(:,105); forldhp = zrv(:,106); forldmp = zrv(:,107); forldlp = zrv(:,108)
      forlntp = zrv(:,109); forlnhp = zrv(:,110); forlnmp = zrv(:,111); forlnlp = zrv(:,112)
      foridtp = zrv(:,113); foridhp = zrv(:,114); foridmp = zrv(:,115); foridlp = zrv(:,116)
      forintp = zrv(:,117); forinhp = zrv(:,118); forinmp = zrv(:,119); forinlp = zrv(:,120)
#endif
      if (do_drfband .and. st == 0) then
         drband(1:ncol,1:nbndsw) = zdr; dfband(1:ncol,1:nbndsw) = zdf
      end if
      ! the reference reports failures through MAPL's RC convention (_FAIL / _RETURN(_SUCCESS), rrtmg_sw_rad.F90:365-383)
      if (present(RC)) then
         RC = st
         if (st /= 0) call geosrad_warn('rrtmg_sw')
      else if (st /= 0) then
         call geosrad_fail('rrtmg_sw')
      end if
   end subroutine rrtmg_sw
end module rrtmg_sw_rad

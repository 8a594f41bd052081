! satsim_shims.F90 -- drop-in EXTERNAL subroutines with the reference's names and exact argument lists for the two fixed-form files of
! GEOSsatsim_GridComp that COSP calls for the ISCCP simulator; the bodies call the C ABI of include/geosrad_satsim.h.  With this file
! linked in place of scops.f and icarus.f (congvec.f is included by scops.f only), cosp.F90 (call at :397) and
! cosp_isccp_simulator.F90 (call at :74-80) compile and link unchanged.
!   scops    scops.f:1-2     subroutine scops(npoints,nlev,ncol,seed,cc,conv,overlap,frac_out,ncolprint)
!   icarus   icarus.f:1-33   SUBROUTINE ICARUS(debug,debugcol,npoints,sunlit,nlev,ncol,pfull,phalf,qv,cc,conv,dtau_s,dtau_c,top_height,
!                            top_height_direction,overlap,frac_out,skt,emsfc_lw,at,dem_s,dem_c,fq_isccp,totalcldarea,meanptop,meantaucld,
!                            meanalbedocld,meantb,meantbclr,boxtau,boxptop)
! debug, debugcol and ncolprint are accepted and ignored: the printing is not part of the port.  Where icarus.f:448-454 prints
! 'Input variable out of range' and STOPs, geosrad_fail stops with the library's message.
! These are the host-array entry points (one round trip over PCIe a call, chunked by geosrad_set_chunk).  A GridComp that keeps its
! fields on the device calls geosrad_isccp_dev instead of COSP (INTEGRATION.md).
module geosrad_satsim_c
   use iso_c_binding
   implicit none
   interface
      integer(c_int) function geosrad_scops(ctx, npoints, nlev, ncol, seed, cc, conv, overlap, frac_out) bind(C, name='geosrad_scops')
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx, seed, cc, conv, frac_out
         integer(c_int), value :: npoints, nlev, ncol, overlap
      end function
      integer(c_int) function geosrad_icarus(ctx, npoints, sunlit, nlev, ncol, pfull, phalf, qv, cc, conv, dtau_s, dtau_c, top_height, &
            top_height_direction, overlap, frac_out, skt, emsfc_lw, at, dem_s, dem_c, fq_isccp, totalcldarea, meanptop, meantaucld, &
            meanalbedocld, meantb, meantbclr, boxtau, boxptop) bind(C, name='geosrad_icarus')
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: ctx, sunlit, pfull, phalf, qv, cc, conv, dtau_s, dtau_c, frac_out, skt, at, dem_s, dem_c, fq_isccp, totalcldarea, &
            meanptop, meantaucld, meanalbedocld, meantb, meantbclr, boxtau, boxptop
         integer(c_int), value :: npoints, nlev, ncol, top_height, top_height_direction, overlap
         real(c_double), value :: emsfc_lw
      end function
   end interface
end module geosrad_satsim_c

subroutine scops(npoints,nlev,ncol,seed,cc,conv,overlap,frac_out,ncolprint)
   use iso_c_binding
   use geosrad_c, only: geosrad_ctx_handle, geosrad_fail
   use geosrad_satsim_c, only: geosrad_scops
   implicit none
   INTEGER npoints, nlev, ncol, overlap, ncolprint
   INTEGER, target :: seed(npoints)
   REAL, target :: cc(npoints,nlev), conv(npoints,nlev)
   REAL, target :: frac_out(npoints,ncol,nlev)
   integer(c_int) :: rc
   rc = geosrad_scops(geosrad_ctx_handle(), int(npoints,c_int), int(nlev,c_int), int(ncol,c_int), c_loc(seed), c_loc(cc), c_loc(conv), &
      int(overlap,c_int), c_loc(frac_out))
   if (rc /= 0) call geosrad_fail('scops')
end subroutine scops

SUBROUTINE ICARUS(debug,debugcol,npoints,sunlit,nlev,ncol,pfull,phalf,qv,cc,conv,dtau_s,dtau_c,top_height,top_height_direction,overlap, &
      frac_out,skt,emsfc_lw,at,dem_s,dem_c,fq_isccp,totalcldarea,meanptop,meantaucld,meanalbedocld,meantb,meantbclr,boxtau,boxptop)
   use iso_c_binding
   use geosrad_c, only: geosrad_ctx_handle, geosrad_fail
   use geosrad_satsim_c, only: geosrad_icarus
   implicit none
   integer debug, debugcol
   INTEGER npoints, nlev, ncol
   INTEGER, target :: sunlit(npoints)
   REAL, target :: pfull(npoints,nlev), phalf(npoints,nlev+1), qv(npoints,nlev), cc(npoints,nlev), conv(npoints,nlev)
   REAL, target :: dtau_s(npoints,nlev), dtau_c(npoints,nlev)
   INTEGER overlap, top_height, top_height_direction
   REAL, target :: skt(npoints)
   REAL emsfc_lw
   REAL, target :: at(npoints,nlev), dem_s(npoints,nlev), dem_c(npoints,nlev)
   REAL, target :: frac_out(npoints,ncol,nlev)
   REAL, target :: fq_isccp(npoints,7,7), totalcldarea(npoints), meanptop(npoints), meantaucld(npoints), meanalbedocld(npoints)
   REAL, target :: meantb(npoints), meantbclr(npoints), boxtau(npoints,ncol), boxptop(npoints,ncol)
   integer(c_int) :: rc
   rc = geosrad_icarus(geosrad_ctx_handle(), int(npoints,c_int), c_loc(sunlit), int(nlev,c_int), int(ncol,c_int), c_loc(pfull), c_loc(phalf), &
      c_loc(qv), c_loc(cc), c_loc(conv), c_loc(dtau_s), c_loc(dtau_c), int(top_height,c_int), int(top_height_direction,c_int), &
      int(overlap,c_int), c_loc(frac_out), c_loc(skt), real(emsfc_lw,c_double), c_loc(at), c_loc(dem_s), c_loc(dem_c), c_loc(fq_isccp), &
      c_loc(totalcldarea), c_loc(meanptop), c_loc(meantaucld), c_loc(meanalbedocld), c_loc(meantb), c_loc(meantbclr), c_loc(boxtau), &
      c_loc(boxptop))
   if (rc /= 0) call geosrad_fail('icarus')
END SUBROUTINE ICARUS

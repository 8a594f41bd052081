! misr_modis_shims.F90 -- a drop-in EXTERNAL subroutine with the reference's name and exact argument list for the fixed-form file of
! GEOSsatsim_GridComp that COSP calls for the MISR simulator; the body calls the C ABI of include/geosrad_misr_modis.h.  With this file
! linked in place of MISR_simulator.f, cosp_misr_simulator.F90 (call at :72-74) compiles and links unchanged.
!   MISR_simulator   MISR_simulator.f:24-39   SUBROUTINE MISR_simulator(npoints,nlev,ncol,sunlit,zfull,at,dtau_s,dtau_c,frac_out,
!                                             missing_value,fq_MISR_TAU_v_CTH,dist_model_layertops,MISR_mean_ztop,MISR_cldarea)
! What the reference does with the first and the last point of a call (the pattern matcher of :314-335, MISR_mean_ztop(npoints) of :460)
! it does here, for the call as a whole.  ncol = 1 stops with the library's message: the reference then scans the points serially.
! This is the host-array entry point (one round trip over PCIe a call, chunked by geosrad_set_chunk); geosrad_misr_dev takes device
! pointers and the byte mask geosrad_scops_dev leaves (INTEGRATION.md).
!   geosrad_modis_simulator   a batched call for the body of COSP_Modis_Simulator (cosp_modis_simulator.F90:69-296) on gridbox-level
!                             arrays from the top of the atmosphere down.  mod_modis_sim itself gets no drop-in: its modis_L2_simulator
!                             takes one point a call with assumed-shape sub-column arrays, which would be a kernel launch a point.
module geosrad_misr_modis_c
   use iso_c_binding
   implicit none
   interface
      integer(c_int) function geosrad_misr(ctx, npoints, nlev, ncol, sunlit, zfull, at, dtau_s, dtau_c, frac_out, missing_value, &
            fq_MISR_TAU_v_CTH, dist_model_layertops, MISR_mean_ztop, MISR_cldarea) bind(C, name='geosrad_misr')
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: ctx, sunlit, zfull, at, dtau_s, dtau_c, frac_out, fq_MISR_TAU_v_CTH, dist_model_layertops, MISR_mean_ztop, MISR_cldarea
         integer(c_int), value :: npoints, nlev, ncol
         real(c_double), value :: missing_value
      end function
      integer(c_int) function geosrad_misr_dev(ctx, stream, npoints, nlev, ncol, sunlit, zfull, at, dtau_s, dtau_c, frac_out_u8, missing_value, &
            fq_MISR_TAU_v_CTH, dist_model_layertops, MISR_mean_ztop, MISR_cldarea) bind(C, name='geosrad_misr_dev')
         import :: c_int, c_ptr, c_double
         type(c_ptr), value :: ctx, stream, sunlit, zfull, at, dtau_s, dtau_c, frac_out_u8, fq_MISR_TAU_v_CTH, dist_model_layertops, MISR_mean_ztop, &
            MISR_cldarea
         integer(c_int), value :: npoints, nlev, ncol
         real(c_double), value :: missing_value
      end function
      integer(c_int) function geosrad_modis(ctx, npoints, nlev, ncol, sunlit, t, p, ph, dtau_s, dtau_c, frac_out, mr_lsliq, mr_lsice, mr_cvliq, &
            mr_cvice, reff_lsliq, reff_lsice, reff_cvliq, reff_cvice, isccp_boxtau, isccp_boxptop, modis_mean, modis_hist, phase, ctp, tau, &
            size) bind(C, name='geosrad_modis')
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx, sunlit, t, p, ph, dtau_s, dtau_c, frac_out, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, reff_lsliq, reff_lsice, &
            reff_cvliq, reff_cvice, isccp_boxtau, isccp_boxptop, modis_mean, modis_hist, phase, ctp, tau, size
         integer(c_int), value :: npoints, nlev, ncol
      end function
   end interface
   ! columns of modis_mean: the GEOSRAD_MODIS_* indices of include/geosrad_misr_modis.h plus one
   integer, parameter :: GEOSRAD_MODIS_NMEAN = 17
end module geosrad_misr_modis_c

SUBROUTINE MISR_simulator(npoints,nlev,ncol,sunlit,zfull,at,dtau_s,dtau_c,frac_out,missing_value,fq_MISR_TAU_v_CTH,dist_model_layertops, &
      MISR_mean_ztop,MISR_cldarea)
   use iso_c_binding
   use geosrad_c, only: geosrad_ctx_handle, geosrad_fail
   use geosrad_misr_modis_c, only: geosrad_misr
   implicit none
   INTEGER npoints, nlev, ncol
   INTEGER, target :: sunlit(npoints)
   REAL, target :: zfull(npoints,nlev), at(npoints,nlev), dtau_s(npoints,nlev), dtau_c(npoints,nlev)
   REAL, target :: frac_out(npoints,ncol,nlev)
   REAL missing_value
   REAL, target :: fq_MISR_TAU_v_CTH(npoints,7,16), dist_model_layertops(npoints,16), MISR_cldarea(npoints), MISR_mean_ztop(npoints)
   integer(c_int) :: rc
   rc = geosrad_misr(geosrad_ctx_handle(), int(npoints,c_int), int(nlev,c_int), int(ncol,c_int), c_loc(sunlit), c_loc(zfull), c_loc(at), &
      c_loc(dtau_s), c_loc(dtau_c), c_loc(frac_out), real(missing_value,c_double), c_loc(fq_MISR_TAU_v_CTH), c_loc(dist_model_layertops), &
      c_loc(MISR_mean_ztop), c_loc(MISR_cldarea))
   if (rc /= 0) call geosrad_fail('MISR_simulator')
END SUBROUTINE MISR_simulator

! COSP_Modis_Simulator's work on gridbox-level arrays (npoints,nlev), level 1 the top: ph (npoints,nlev+1); frac_out the real mask of scops;
! isccp_boxptop (npoints,ncol) in hPa from icarus; modis_mean (npoints,17) in modis_L3_simulator's argument order, modis_hist
! (npoints,7,7) as COSP leaves it (tau index 1 R_UNDEF, pressure from the surface up).  The convective arrays are mandatory here: pass zeros.
subroutine geosrad_modis_simulator(npoints, nlev, ncol, sunlit, t, p, ph, dtau_s, dtau_c, frac_out, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, &
      reff_lsliq, reff_lsice, reff_cvliq, reff_cvice, isccp_boxptop, modis_mean, modis_hist)
   use iso_c_binding
   use geosrad_c, only: geosrad_ctx_handle, geosrad_fail
   use geosrad_misr_modis_c, only: geosrad_modis
   implicit none
   integer npoints, nlev, ncol
   integer, target :: sunlit(npoints)
   real, target :: t(npoints,nlev), p(npoints,nlev), ph(npoints,nlev+1), dtau_s(npoints,nlev), dtau_c(npoints,nlev)
   real, target :: frac_out(npoints,ncol,nlev)
   real, target :: mr_lsliq(npoints,nlev), mr_lsice(npoints,nlev), mr_cvliq(npoints,nlev), mr_cvice(npoints,nlev)
   real, target :: reff_lsliq(npoints,nlev), reff_lsice(npoints,nlev), reff_cvliq(npoints,nlev), reff_cvice(npoints,nlev)
   real, target :: isccp_boxptop(npoints,ncol), modis_mean(npoints,17), modis_hist(npoints,7,7)
   integer(c_int) :: rc
   rc = geosrad_modis(geosrad_ctx_handle(), int(npoints,c_int), int(nlev,c_int), int(ncol,c_int), c_loc(sunlit), c_loc(t), c_loc(p), c_loc(ph), &
      c_loc(dtau_s), c_loc(dtau_c), c_loc(frac_out), c_loc(mr_lsliq), c_loc(mr_lsice), c_loc(mr_cvliq), c_loc(mr_cvice), c_loc(reff_lsliq), &
      c_loc(reff_lsice), c_loc(reff_cvliq), c_loc(reff_cvice), c_null_ptr, c_loc(isccp_boxptop), c_loc(modis_mean), c_loc(modis_hist), &
      c_null_ptr, c_null_ptr, c_null_ptr, c_null_ptr)
   if (rc /= 0) call geosrad_fail('geosrad_modis_simulator')
end subroutine geosrad_modis_simulator

! lidar_shims.F90 -- the lidar simulator of GEOSsatsim_GridComp's COSP for a Fortran caller; the body calls the C ABI of
! include/geosrad_lidar.h.
!   geosrad_lidar_simulator   a batched call for COSP_LIDAR (cosp_lidar.F90:44-82) and diag_lidar (actsim/lmd_ipsl_stats.F90:34-179, as
!                             cosp_stats.F90:126-140 calls it and leaves its results) on gridbox-level arrays from the top of the
!                             atmosphere down.  lidar_simulator itself gets no drop-in: COSP_LIDAR calls it once per sub-column
!                             (cosp_lidar.F90:63-80) on arrays it cuts out of sghydro%mr_hydro, which would be ncol round trips over PCIe
!                             and ncol launches a call, with diag_lidar left on the host.
! This is the host-array entry point (one round trip over PCIe a call, chunked by geosrad_set_chunk); geosrad_lidar_dev takes device
! pointers and the byte mask geosrad_scops_dev leaves, geosrad_cosp_lidar_dev GEOS's own fields (INTEGRATION.md).
module geosrad_lidar_c
   use iso_c_binding
   implicit none
   interface
      integer(c_int) function geosrad_lidar(ctx, npoints, nlev, ncol, ice_type, p, t, presf, pplay, frac_out, mr_lsliq, mr_lsice, mr_cvliq, &
            mr_cvice, reff_lsliq, reff_lsice, reff_cvliq, reff_cvice, land, lidarcld, cldlayer, cfad_sr, parasolrefl, pmol, beta_tot, tau_tot, &
            refl) bind(C, name='geosrad_lidar')
         import :: c_int, c_ptr
         type(c_ptr), value :: ctx, p, t, presf, pplay, frac_out, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, reff_lsliq, reff_lsice, reff_cvliq, &
            reff_cvice, land, lidarcld, cldlayer, cfad_sr, parasolrefl, pmol, beta_tot, tau_tot, refl
         integer(c_int), value :: npoints, nlev, ncol, ice_type
      end function
   end interface
   ! columns of cldlayer: the GEOSRAD_LIDAR_* indices of include/geosrad_lidar.h plus one
   integer, parameter :: GEOSRAD_LIDAR_LOW = 1, GEOSRAD_LIDAR_MID = 2, GEOSRAD_LIDAR_HIGH = 3, GEOSRAD_LIDAR_TOTAL = 4
end module geosrad_lidar_c

! p, t, pplay, the contents and the radii (npoints,nlev), level 1 the top; presf (npoints,nlev+1), the layer edges from the top; frac_out the
! real mask of scops; land (npoints) 0 ocean, 1 land.  lidarcld, pmol (npoints,nlev); cldlayer (npoints,4) low, mid, high, total; cfad_sr
! (npoints,15,nlev); parasolrefl (npoints,5); -1.0E30 where COSP leaves R_UNDEF.  The convective arrays are mandatory here: pass zeros.
subroutine geosrad_lidar_simulator(npoints, nlev, ncol, ice_type, p, t, presf, pplay, frac_out, mr_lsliq, mr_lsice, mr_cvliq, mr_cvice, &
      reff_lsliq, reff_lsice, reff_cvliq, reff_cvice, land, lidarcld, cldlayer, cfad_sr, parasolrefl, pmol)
   use iso_c_binding
   use geosrad_c, only: geosrad_ctx_handle, geosrad_fail
   use geosrad_lidar_c, only: geosrad_lidar
   implicit none
   integer npoints, nlev, ncol, ice_type
   real, target :: p(npoints,nlev), t(npoints,nlev), presf(npoints,nlev+1), pplay(npoints,nlev)
   real, target :: frac_out(npoints,ncol,nlev)
   real, target :: mr_lsliq(npoints,nlev), mr_lsice(npoints,nlev), mr_cvliq(npoints,nlev), mr_cvice(npoints,nlev)
   real, target :: reff_lsliq(npoints,nlev), reff_lsice(npoints,nlev), reff_cvliq(npoints,nlev), reff_cvice(npoints,nlev)
   real, target :: land(npoints), lidarcld(npoints,nlev), cldlayer(npoints,4), cfad_sr(npoints,15,nlev), parasolrefl(npoints,5), pmol(npoints,nlev)
   integer(c_int) :: rc
   rc = geosrad_lidar(geosrad_ctx_handle(), int(npoints,c_int), int(nlev,c_int), int(ncol,c_int), int(ice_type,c_int), c_loc(p), c_loc(t), &
      c_loc(presf), c_loc(pplay), c_loc(frac_out), c_loc(mr_lsliq), c_loc(mr_lsice), c_loc(mr_cvliq), c_loc(mr_cvice), c_loc(reff_lsliq), &
      c_loc(reff_lsice), c_loc(reff_cvliq), c_loc(reff_cvice), c_loc(land), c_loc(lidarcld), c_loc(cldlayer), c_loc(cfad_sr), c_loc(parasolrefl), &
      c_loc(pmol), c_null_ptr, c_null_ptr, c_null_ptr)
   if (rc /= 0) call geosrad_fail('geosrad_lidar_simulator')
end subroutine geosrad_lidar_simulator

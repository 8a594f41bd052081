! driver_gases.f90 -- calls the reference's own `gases` (quickbeam/gases.f90) for every volume and `path_integral` of module math_lib
! (quickbeam/math_lib.f90, with mrgrnk.f90 and array_lib.f90) for every gate, the way radar_simulator.f90:478-480 does - the temperature
! arrives in Celsius and gets its + 273.15 here, the integral runs from the radar's first gate to the gate before the volume - all compiled
! unmodified from GEOSsatsim_GridComp by make_fixture.py, never copied.  One plain build: quickbeam is real*8 throughout.
! in.bin: nprof, ngate (integers); freq; p_matrix (hPa), t_matrix (C), rh_matrix (%), hgt_matrix (km), each (nprof,ngate) real*8, the
! radar's first gate first (make_fixture.py does cosp_radar.F90:136-139's conversions and order_data's flip).  out.bin: g_vol, g_to_vol
! (nprof,ngate) real*8.
program driver_gases
  use math_lib, only: path_integral
  implicit none
  integer :: nprof, ngate, pr, k
  real*8 :: freq
  real*8, external :: gases
  real*8, allocatable :: p(:,:), t(:,:), rh(:,:), hgt(:,:), g_vol(:), g_all(:,:), g_to_vol(:,:)
  open(10, file='in.bin', access='stream', form='unformatted', status='old')
  read(10) nprof, ngate
  allocate(p(nprof,ngate), t(nprof,ngate), rh(nprof,ngate), hgt(nprof,ngate), g_vol(ngate), g_all(nprof,ngate), g_to_vol(nprof,ngate))
  read(10) freq, p, t, rh, hgt
  close(10)
  do pr = 1, nprof
     g_vol = 0
     do k = 1, ngate
        g_vol(k) = gases(p(pr,k), t(pr,k)+273.15, rh(pr,k), freq)
        g_to_vol(pr,k) = path_integral(g_vol, hgt(pr,:), 1, k-1)
     end do
     g_all(pr,:) = g_vol
  end do
  open(11, file='out.bin', access='stream', form='unformatted', status='replace')
  write(11) g_all, g_to_vol
  close(11)
end program

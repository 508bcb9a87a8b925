!==============================================================================
! cooling_fine.f90 of the ramses_amd patch directory.
!
! Shadows hydro/cooling_fine.f90 (cooling_fine -> *_reference by #define +
! #include; coolfine1 and cmp_Eddington_tensor stay the reference's).  In a run
! with a barotropic equation of state of CONSTANT temperature and without
! cooling (ramses_amd_iface: ramses_amd_eos_on -- RAMSES_AMD_EOS=1, the form
! 'isothermal', or 'legacy' with g_star = 1) the routine only rewrites the total
! energy of the level's leaf cells; while the hydro state is device-resident that
! runs on the resident state (csrc/eos_core.hpp).  Otherwise the reference.
!==============================================================================
#define cooling_fine cooling_fine_reference
#include "hydro/cooling_fine.f90"
#undef cooling_fine

subroutine cooling_fine_amd(ilevel,on_device,on_reference)
  use amr_commons
  use hydro_commons
  use ramses_amd_iface
  implicit none
  integer::ilevel
  logical::on_device,on_reference
  !--------------------------------------------------------------------------
  ! Same contract as the reference (hydro/cooling_fine.f90:1-45 with :576-579):
  ! uold(:,ndim+2) of the leaf cells of the level's active octs becomes
  ! T2min*nH/scale_T2/(gamma-1) + ekk; nothing else is written.
  ! AMR-resident, then the resident brick, then the MPI-resident brick, else
  ! the reference.
  !--------------------------------------------------------------------------
  type(ramses_amd_hydro_params)::p
  integer::rc

  on_device=.false.
  on_reference=.false.
  ! the reference's own early return (:17)
  if(numbtot(1,ilevel)==0)return
  if(ramses_amd_eos_on())then
     if(ramses_amd_amr_resident())then
        call ramses_amd_amr_ensure()
        call ramses_amd_fill_hydro_params(p)
        rc=ramses_amd_amrres_cooling_fine(p,active(ilevel)%ngrid,ramses_amd_octs(ilevel))
        if(rc/=0)call ramses_amd_fatal('cooling_fine')
        on_device=.true.
        return
     end if
     if(ramses_amd_resident())then
        if(verbose)write(*,111)ilevel
        call ramses_amd_fill_hydro_params(p)
        rc=ramses_amd_resident_cooling_fine_f90(p,ilevel)
        if(rc/=0)call ramses_amd_fatal('cooling_fine')
        on_device=.true.
        return
     end if
     if(ramses_amd_mpi_resident())then
        call ramses_amd_fill_hydro_params(p)
        rc=ramses_amd_mpires_cooling_fine(p)
        if(rc/=0)call ramses_amd_fatal('cooling_fine')
        on_device=.true.
        return
     end if
  end if
  call cooling_fine_reference(ilevel)
  on_reference=.true.

111 format('   Entering cooling_fine (MI355X) for level',i2)

end subroutine cooling_fine_amd

subroutine cooling_fine(ilevel)
  use ramses_amd_iface
  implicit none
  integer::ilevel
  integer(8)::t0
  logical::on_device,on_reference
  call ramses_amd_tic(t0)
  call cooling_fine_amd(ilevel,on_device,on_reference)
  ! (an empty level is neither)
  if(on_device)call ramses_amd_toc('cooling_fine (device, barotropic)',ilevel,t0)
  if(on_reference)call ramses_amd_toc('cooling_fine',ilevel,t0)
end subroutine cooling_fine

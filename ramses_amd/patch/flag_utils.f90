!==============================================================================
! flag_utils.f90 of the ramses_amd patch directory.
!
! Shadows amr/flag_utils.f90: flag_fine, userflag_fine, smooth_fine, ensure_ref_rules, geometry_refine, ... stay the
! reference's, poisson_refine is replaced.  (flag_utils_ref.f90: the reference's file with the DEFINITION of poisson_refine
! renamed to poisson_refine_reference, generated into the build directory by prepare.sh -- its caller userflag_fine lives in
! the same file, where the preprocessor rename of the other shims would catch the call as well.)
! poisson_refine has two branches that read the hydro state: the density threshold of a run without self-gravity
! (amr/flag_utils.f90:480-485: uold(:,1) >= m_refine*d_scale) and the scalar cut of the initial refinement (:465-470:
! uold(:,ivar_refine)/uold(:,1) > var_cut_refine).  flag_fine runs at the end of amr_step, after the level's hydro update
! and before refine_fine brings the levels home, so while the device holds the state the host array is stale there: the
! criterion is then evaluated on the resident state, once per level (ramses_amd_amrres_refine_flag), and the calls of
! userflag_fine's loop (nvector cells of one octant at a time) look their cells up in the list that came back.  The cpu_map2
! branches (:457-464) and every call made while the host holds the state run the reference's code.
!==============================================================================
#include "flag_utils_ref.f90"

subroutine poisson_refine(ind_cell,ok,ncell,ilevel)
  use amr_commons
  use pm_commons
  use hydro_commons
  use poisson_commons
  use ramses_amd_iface
  implicit none
  integer::ncell,ilevel
  integer,dimension(1:nvector)::ind_cell
  logical,dimension(1:nvector)::ok
  integer::i,k,rc,ncache,nx_loc,mode
  real(dp)::d_scale,scale,dx,dx_loc,vol_loc
  type(ramses_amd_hydro_params)::p
  type(ramses_amd_refine_crit)::crit
  integer(8)::t0
  ! the cells of the level under way that pass the criterion: hit(icell) /= 0
  integer(kind=1),allocatable,dimension(:),save::hit
  integer,allocatable,dimension(:),save::cells
  integer,save::nhit=0

  ! which branch of the reference reads uold here (0: none)
  mode=0
  if(poisson)then
     if(init.and.ivar_refine>0)mode=2
  else
     if(hydro)mode=1
  end if
  if(mode>0.and.ncell>0)then
     if(.not.ramses_amd_amr_resident())mode=0
  end if
  if(mode>0.and.ncell>0)then
     if(ramses_amd_amrres_active()==0)mode=0
  end if
  if(mode==0.or.ncell<=0)then
     call poisson_refine_reference(ind_cell,ok,ncell,ilevel)
     return
  end if

  ! userflag_fine starts every level at the first cell of its first oct (amr/flag_utils.f90:352-368): evaluate the level
  if(ind_cell(1)==ncoarse+active(ilevel)%igrid(1))then
     call ramses_amd_tic(t0)
     call ramses_amd_amr_ensure()
     call ramses_amd_fill_hydro_params(p)
     if(.not.allocated(hit))then
        allocate(hit(1:ncoarse+twotondim*ngridmax))
        hit=0
     end if
     do k=1,nhit
        hit(cells(k))=0
     end do
     ncache=active(ilevel)%ngrid
     if(allocated(cells))then
        if(size(cells)<twotondim*ncache)deallocate(cells)
     end if
     if(.not.allocated(cells))allocate(cells(1:twotondim*max(ncache,1)))
     crit%err_grad_d=-1.0d0; crit%err_grad_p=-1.0d0; crit%err_grad_u=-1.0d0
     crit%floor_d=dble(floor_d); crit%floor_p=dble(floor_p); crit%floor_u=dble(floor_u)
     crit%n_jeans=-1.0d0; crit%tail_pix=0.0d0; crit%factG=1.0d0
     crit%thr=0.0d0; crit%var_cut_refine=0.0d0; crit%ivar_refine=0
     crit%thr_mode=mode
     if(mode==1)then
        ! amr/flag_utils.f90:448-452,481-483
        nx_loc=(icoarse_max-icoarse_min+1)
        scale=boxlen/dble(nx_loc)
        dx=0.5d0**ilevel
        dx_loc=dx*scale
        vol_loc=dx_loc**3
        d_scale=mass_sph/vol_loc
        crit%thr=m_refine(ilevel)*d_scale
     else
        crit%ivar_refine=ivar_refine
        crit%var_cut_refine=var_cut_refine
     end if
     rc=ramses_amd_amrres_refine_flag(p,ncache,ramses_amd_octs(ilevel),crit,cells,nhit)
     if(rc/=0)call ramses_amd_fatal('poisson_refine')
     do k=1,nhit
        hit(cells(k))=1
     end do
     call ramses_amd_toc('poisson_refine (shim: kernel + list)',ilevel,t0)
  end if
  do i=1,ncell
     ok(i)=ok(i).or.(hit(ind_cell(i))/=0)
  end do
end subroutine poisson_refine

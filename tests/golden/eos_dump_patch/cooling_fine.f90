!==============================================================================
! tests/golden/eos_dump_patch/cooling_fine.f90 -- TEST INFRASTRUCTURE ONLY.
!
! A RAMSES patch directory (same mechanism as oracle/dump_patch) that wraps the
! UNMODIFIED reference cooling_fine and dumps, around the calls asked for, uold
! and son of the cells of the level's active octs: tests/golden/make_golden_eos.py
! runs the program built with it and turns the dumps into tests/golden/eos_ref.npz.
! Nothing of the reference is restated here.
!
! RAMSES_DUMP_CALLS = comma separated 1-based call numbers of cooling_fine to dump
!==============================================================================
#define cooling_fine cooling_fine_reference
#include "hydro/cooling_fine.f90"
#undef cooling_fine

subroutine cooling_fine(ilevel)
  use amr_commons
  use hydro_commons
  implicit none
  integer::ilevel
  integer,save::ncall=0
  logical::dump
  character(len=256)::val
  character(len=16)::tag
  integer::stat
  if(numbtot(1,ilevel)==0)return
  ncall=ncall+1
  dump=.false.
  call get_environment_variable('RAMSES_DUMP_CALLS',val,status=stat)
  if(stat==0)then
     write(tag,'(I0)')ncall
     val=','//trim(adjustl(val))//','
     dump=index(val,','//trim(tag)//',')>0
  end if
  if(dump)call dump_cooling('in',ilevel,ncall)
  call cooling_fine_reference(ilevel)
  if(dump)call dump_cooling('out',ilevel,ncall)
end subroutine cooling_fine

subroutine dump_cooling(what,ilevel,ncall)
  use amr_commons
  use hydro_commons
  implicit none
  character(len=*)::what
  integer::ilevel,ncall,i,ind,ivar,ngrid
  character(len=64)::fname
  real(dp)::scale_l,scale_t,scale_d,scale_v,scale_nH,scale_T2
  write(fname,'(A,I4.4,A,A,A)')'cooling_',ncall,'_',trim(what),'.bin'
  open(unit=77,file=trim(fname),form='unformatted',access='stream',status='replace')
  ngrid=active(ilevel)%ngrid
  call units(scale_l,scale_t,scale_d,scale_v,scale_nH,scale_T2)
  write(77)ilevel,ngrid,nvar
  write(77)gamma,smallr,scale_nH,scale_T2,T2_eos,T2_star,g_star,jeans_ncells
  ! [nvar][8][ngrid], then son [8][ngrid]
  do ivar=1,nvar
     do ind=1,twotondim
        write(77)(uold(ncoarse+(ind-1)*ngridmax+active(ilevel)%igrid(i),ivar),i=1,ngrid)
     end do
  end do
  do ind=1,twotondim
     write(77)(son(ncoarse+(ind-1)*ngridmax+active(ilevel)%igrid(i)),i=1,ngrid)
  end do
  close(77)
end subroutine dump_cooling

#!/bin/bash
# prepare.sh REF GEN -- derived sources of the ramses_amd patch, generated from the reference tree where it lies
# (nothing of it is kept in this repository):
#   GEN/multigrid_fine_commons_ref.f90 = poisson/multigrid_fine_commons.f90 with the DEFINITIONS of make_virtual_mg_dp and
#   make_reverse_mg_dp renamed to *_reference.  Their callers (multigrid_fine, recursive_multigrid_coarse) sit in the same
#   file, so the preprocessor rename the other shims use would rename the calls as well; this way the calls reach the
#   routines of the same name in ramses_amd/patch/multigrid_fine_commons.f90.
#   GEN/flag_utils_ref.f90 = amr/flag_utils.f90 with the DEFINITION of poisson_refine renamed to poisson_refine_reference, for
#   the same reason: its caller userflag_fine sits in the same file and must reach ramses_amd/patch/flag_utils.f90.
set -e
REF=$1; GEN=$2
mkdir -p "$GEN"
derive() { # source (under REF), output (under GEN), names (a|b), expected number of renamed "subroutine" lines
  sed -E "s/(subroutine[ ]+)($3)\b/\1\2_reference/I" "$REF/$1" > "$GEN/$2.tmp"
  # (keep the time stamp unless the content changed: the build compiles what is newer than its object)
  if ! cmp -s "$GEN/$2.tmp" "$GEN/$2" 2>/dev/null; then
    mv "$GEN/$2.tmp" "$GEN/$2"
  else
    rm -f "$GEN/$2.tmp"
  fi
  grep -c -i -E "subroutine[ ]+($3)_reference" "$GEN/$2" | grep -qx "$4"
}
derive poisson/multigrid_fine_commons.f90 multigrid_fine_commons_ref.f90 "make_virtual_mg_dp|make_reverse_mg_dp" 4
derive amr/flag_utils.f90 flag_utils_ref.f90 "poisson_refine" 2

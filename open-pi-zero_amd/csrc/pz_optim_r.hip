// The second object of pz_optim.hip: pz_adamw8bit_r and pz_adamw_r (see the note above pz_adamw8bit there).
#define PZ_OPTIM_ROUNDING 1
#include "pz_optim.hip"

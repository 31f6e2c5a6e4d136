// states.hip -- the kernels that work on caller-supplied state vectors, as one object (states.o).  Each file below is a
// translation unit of its own (it compiles alone and uses no name of another .hip file); what they share is state_sweep.h.
#include "import_states.hip"
#include "thermal.hip"
#include "krylov.hip"
#include "gram.hip"
#include "reduced.hip"

#define CIAO_T float
#include "colmom_launch.inc"

#define CIAO_T float
#include "mstat_launch.inc"

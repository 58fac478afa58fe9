#define CIAO_T float
#include "mscore_launch.inc"

#define CIAO_T float
#include "list_launch.inc"

#include "gramcdg_launch.inc"
